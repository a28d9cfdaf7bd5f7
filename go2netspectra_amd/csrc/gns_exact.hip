// gns_exact.hip -- MI355X engine for Go2NetSpectra's exact aggregator
// (internal/engine/impl/exact/task.go): per-flow PacketCount, ByteCount,
// StartTime (first packet) and EndTime (last packet, in stream order).
//
// Keys: the reference keys flows by the STRING strings.Join(fields, "-")
// with IPs printed by net.IP.String() (generateKeyAndFields, task.go:330-366).
// Two IPs print the same exactly when their 16-byte forms (To16) are equal:
// IPv4 (4-byte) and IPv4-mapped IPv6 both print as a dotted quad, every other
// IPv6 prints its 16 bytes.  The engine therefore keys flows by the key bytes
// of the sketch layout (task.go:265-300) with every IP field in To16 form, in
// the flow dictionary of gns_keys.cuh (full key bytes, exact compare).
//
// Nothing in task.go:124-149 depends on packet order except which packet is
// the flow's first and last: PacketCount / ByteCount are sums, StartTime is
// the timestamp of the packet with the smallest stream index, EndTime that of
// the largest.  So every path below produces per-flow (count, bytes, min
// index, max index) contributions, merged with add / min / max, and the
// timestamps are looked up once per batch from the merged indices.
//
//   X1  k_ex_extract   parse -> To16 tuple -> key -> flow id (dictionary);
//                      packets of the batch's designated heavy flows (the 512
//                      flows with the most packets so far) are aggregated in
//                      LDS per block (per-block partials), every other packet
//                      writes a 64-bit word (flow id | packet index | length)
//   X1b k_ex_resolve   re-probe packets parked on a same-launch claim
//   H   k_ex_hot_reduce  the partials of each designated flow -> flow state
//   P   k_ex_phist / k_ex_pscan_* / k_ex_pscatter / k_ex_pagg  X1 writes the
//                      words of the other flows (the tail: about 35% of a
//                      Zipf(1.1) stream) at the start of its block's region; they
//                      are partitioned into 512 bins of consecutive flow ids and
//                      each bin is aggregated in an LDS hash table by one
//                      workgroup, which merges each of its flows once
//   T   k_ex_times     StartTime / EndTime of the flows the batch touched
//   D   k_exh_*        designate the next batch's heavy flows
//   Q   k_exq_aggregate  filtered aggregates of the resident table (gns_ex_aggregate)
//   HH  k_exq_hh_*     flows above a threshold, ordered, cut to a limit (gns_ex_heavy_hitters)
//   A   k_exh_link     a view's rows appended to a history's log (gns_ex_hist_append); Q, HH
//                      and V answer over the log as of a snapshot (gns_ex_hist_*)
//   AR  k_exh_link_rows  host rows appended to the log (gns_ex_hist_append_rows;
//                      HistIndex::check_unique refuses a key that occurs twice in the call)
//   TR  k_exh_trim_*   expired snapshots dropped or folded into a base snapshot: the kept rows
//                      moved into a new log, the head words remapped (gns_ex_hist_trim)
// A Zipf batch touches a flow in many places; per-block LDS aggregation of
// every flow left the tail flows to global atomics, three per packet; sorting
// every packet (rocPRIM radix sort of 100M words) made the sort the largest
// stage.  Designation sends the heavy flows through LDS; the tail needs no
// order at all (add / min / max), only locality by flow id.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <optional>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_merge_sort.hpp>

#include "gns_common.hpp"
#include "gns_exsrc.hpp"
#include "gns_histindex.hpp"
#include "gns_scan.cuh"
#include "gns_xcd.cuh"

namespace gns {

constexpr int kXThreads = 256;

constexpr uint32_t kXChunk = 16384;

// Designated heavy flows: kExHot per batch, looked up by flow id in a 4-way
// table of kExHotTab entries (id << 16 | hot slot; empty = ~0) that X1 keeps in LDS.
#ifndef GNS_EX_HOT_BITS
#define GNS_EX_HOT_BITS 9
#endif
constexpr uint32_t kExHotBits = GNS_EX_HOT_BITS;
constexpr uint32_t kExHot = 1u << kExHotBits;
constexpr uint32_t kExHotTab = 4 * kExHot;
constexpr uint32_t kExHotMinKey = 6 * 8;  // designate only flows with >= 64 packets
// One designated flow in one X1 block: bytes << 15 | packets (a block has at
// most 2^14 packets of < 2^32 bytes, so neither field carries into the other)
// and the largest packet index in the block.  No first-packet index: a flow is
// designated only with >= 64 packets counted, so its first packet is known.
constexpr uint32_t kHotCntBits = 15;
static_assert(kXChunk < (1u << kHotCntBits), "per-block packet count field");
struct ExHotPart {
    unsigned long long cb;
    uint32_t maxp, pad;
};
__device__ __forceinline__ uint32_t exh_group(uint32_t id) { return (id * 0x9E3779B1u) >> (32 - kExHotBits); }
__device__ __forceinline__ int exh_lookup(const unsigned long long *tab, uint32_t id) {
    const ulonglong2 *g = reinterpret_cast<const ulonglong2 *>(tab + exh_group(id) * 4);
    const ulonglong2 a = g[0], b = g[1];
    int h = -1;
    constexpr unsigned long long m = kExHot - 1u;
    h = (b.y >> 16) == id ? (int)(b.y & m) : h;
    h = (b.x >> 16) == id ? (int)(b.x & m) : h;
    h = (a.y >> 16) == id ? (int)(a.y & m) : h;
    h = (a.x >> 16) == id ? (int)(a.x & m) : h;
    return h;
}

struct ExIn {
    InputDesc in;
    const uint8_t *ipver;  // IN_TUPLE: 4 / 6 per packet (NULL -> 4)
    const int64_t *ts;
};

// IPv4 (4-byte net.IP, left-aligned in its slot) -> ::ffff:a.b.c.d, the form
// in which it compares equal to the same address arriving IPv4-mapped.
__device__ __forceinline__ void to16(uint32_t (&tw)[10], uint32_t sver, uint32_t dver) {
    if (sver == 4u) { tw[3] = tw[0]; tw[0] = 0u; tw[1] = 0u; tw[2] = 0xFFFF0000u; }
    if (dver == 4u) { tw[7] = tw[4]; tw[4] = 0u; tw[5] = 0u; tw[6] = 0xFFFF0000u; }
}

// canonical tuple words (load_tuple) -> exact key with To16 IP fields
template <int KIND, int MODE>
__device__ __forceinline__ int ex_key_tw(const ExIn &x, uint32_t K, const uint8_t *s_src, uint64_t p,
                                         uint32_t (&tw)[10], uint32_t (&kw)[GNS_KWMAX]) {
    uint32_t sv, dv;
    if constexpr (KIND == IN_HDR || KIND == IN_REC16) { sv = tw[9] >> 24; dv = (tw[9] >> 16) & 0xFFu; }
    else { sv = dv = x.ipver ? x.ipver[p] : 4u; }
    // a net.IP of neither 4 nor 16 bytes prints as "?<hex>" / "<nil>" (net/ip.go):
    // outside the canonical form, counted as unsupported
    if (sv == 0u || dv == 0u) return PARSE_UNSUPPORTED;
    to16(tw, sv, dv);
    tw[9] &= 0xFFu;
    make_key_m<MODE, GNS_KWMAX>(K, s_src, tw, kw);
    return PARSE_OK;
}

template <int KIND, int MODE>
__device__ __forceinline__ int ex_key(const ExIn &x, uint32_t K, const uint8_t *s_src, uint64_t p,
                                      uint32_t (&kw)[GNS_KWMAX]) {
    uint32_t tw[10];
    const int st = load_tuple<KIND>(x.in, p, tw);
    if (st != PARSE_OK) return st;
    return ex_key_tw<KIND, MODE>(x, K, s_src, p, tw, kw);
}

struct ExArgs {
    ExIn x;
    uint64_t n;
    KeyPlanN kp;
    DictDev D;
    uint32_t epoch;
    uint64_t *sk;        // X2 sort words: flow id | packet index | wire length (SortWord)
    uint32_t none_key;   // flow field of a packet without a flow id (sorts last)
    uint32_t hot_key;    // flow field of a designated flow's packet (none_key + 1: not sorted)
    uint32_t sb, ib;     // SortWord field widths: wire length, packet index
    const unsigned long long *hot_tab;  // [kExHotTab] designated flows
    ExHotPart *hpart;    // [kExHot][nblk] per-block partials
    uint32_t *ccnt;      // [nblk] words X1 wrote at the start of its block's region
    uint32_t nblk;
    uint64_t *pend;
    uint32_t *pend_cnt, *pend_total;
    unsigned long long *stats;  // 0 inserted, 1 dropped, 2 unsupported, 3 dict full
};

// X2 sorts one 64-bit word per packet: flow id in the top bits (the radix sort's
// key range), then the packet index within the batch (ib bits), then the wire
// length (sb bits; a length >= 2^sb - 1 is stored as the escape 2^sb - 1 and
// read back from the batch's length array by X3).  A keys-only sort of 8 bytes
// per packet instead of 4-byte keys with 8-byte values.
__device__ __forceinline__ uint64_t sort_word(uint32_t flow, uint64_t idx, uint32_t size, uint32_t sb,
                                              uint32_t ib) {
    const uint32_t esc = (1u << sb) - 1u;
    return (uint64_t)flow << (ib + sb) | idx << sb | (size < esc ? size : esc);
}

// Home-slot record of a key (issued early; consumed by ex_consume).
__device__ __forceinline__ void ex_probe_issue(const DictDev &D, uint32_t slot, uint4 (&r4)[4]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(D.rec + (size_t)slot * D.RW);
#pragma unroll
    for (int i = 0; i < 4; i++) r4[i] = (4u * i < D.RW) ? q[i] : make_uint4(0, 0, 0, 0);
}

// X1 second half for one packet: resolve the home-slot probe.  A hit gives the
// flow id; a flow displaced from its home slot by another committed key is parked
// (k_ex_resolve walks the rest of the chain in the next launch) instead of
// stalling the wave on dependent probes; an empty home slot is claimed here.
struct ExHotLds {
    const unsigned long long *tab;
    unsigned long long *cb;
    uint32_t *maxp;
};

constexpr uint64_t kNoWord = ~0ull;
// Word of a packet of an undesignated flow, written densely at the start of the
// block's region (ballot + one LDS add per wave); returns its position in the
// region (parked packets record it for k_ex_resolve), or ~0u for no word.
__device__ __forceinline__ uint32_t ex_emit(const ExArgs &a, uint64_t beg, uint64_t w, uint32_t *s_ncold) {
    const bool has = w != kNoWord;
    const uint64_t m = __ballot(has);
    if (!m) return ~0u;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(s_ncold, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    const uint32_t q = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (has) a.sk[beg + q] = w;
    return has ? q : ~0u;
}

// X1 second half for one packet; returns the packet's word (kNoWord: none) and
// whether it is parked (*park: the dictionary slot to resume from).
__device__ __forceinline__ uint64_t ex_consume(const ExArgs &a, uint64_t p, uint64_t beg, bool ok,
                                               const uint32_t (&kw)[GNS_KWMAX], uint32_t K, uint32_t slot0,
                                               const uint4 (&r4)[4], uint32_t sz, uint32_t *s_full,
                                               uint32_t *s_claim, uint32_t &n_ok, const ExHotLds &H,
                                               uint32_t &park) {
    park = ~0u;
    if (!ok) return kNoWord;
    uint32_t rec[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        rec[4 * i] = r4[i].x; rec[4 * i + 1] = r4[i].y; rec[4 * i + 2] = r4[i].z; rec[4 * i + 3] = r4[i].w;
    }
    const uint32_t tag = rec[0];
    bool eq = tag != 0 && tag != a.epoch;
#pragma unroll
    for (int i = 0; i < GNS_KWMAX; i++)
        if ((uint32_t)i < ((K + 3) >> 2)) eq = eq && (rec[1 + i] == kw[i]);
    uint32_t out = slot0;
    int r = DICT_FOUND;
    if (eq) {  // a designated flow: aggregated in LDS, no word to sort
        const int h = exh_lookup(H.tab, out);
        if (h >= 0) {
            const uint32_t lp = (uint32_t)(p - beg);
            atomicAdd(&H.cb[h], (unsigned long long)sz << kHotCntBits | 1ull);
            atomicMax(&H.maxp[h], lp);
            n_ok++;
            return kNoWord;
        }
    } else {
        if (tag == a.epoch) r = DICT_PENDING;                                    // claimed in this launch
        else if (tag != 0) { r = DICT_PENDING; out = (slot0 + 1u) & a.D.mask; }  // displaced
        else r = dict_find_or_claim(a.D, kw, slot0, a.epoch, &out);              // empty: claim
    }
    if (r == DICT_CLAIMED) {
        atomicAdd(s_claim, 1u);
        r = DICT_FOUND;
    }
    if (r == DICT_FULL) {
        atomicAdd(s_full, 1u);
        return kNoWord;
    }
    n_ok++;
    // a parked packet's word keeps none_key until k_ex_resolve fills in its flow id
    if (r != DICT_FOUND) park = out;
    return sort_word(r == DICT_FOUND ? out : a.none_key, p, sz, a.sb, a.ib);
}

// pend entry: packet (14 bits) | word position (14 bits) in the block | slot to resume from
static_assert(kXChunk <= (1u << 14), "pend entries hold 14-bit block offsets");
__device__ __forceinline__ uint64_t pend_entry(uint32_t lp, uint32_t q, uint32_t slot) {
    return (uint64_t)lp << 50 | (uint64_t)q << 36 | slot;
}
__device__ __forceinline__ void ex_emit_park(const ExArgs &a, uint64_t beg, uint64_t p, uint64_t w, uint32_t park,
                                             uint32_t *s_ncold, uint32_t *s_pend) {
    const uint32_t q = ex_emit(a, beg, w, s_ncold);
    if (park != ~0u) a.pend[beg + atomicAdd(s_pend, 1u)] = pend_entry((uint32_t)(p - beg), q, park);
}

template <int KIND, int MODE>
__global__ __launch_bounds__(kXThreads) void k_ex_extract(ExArgs a) {
    __shared__ uint8_t s_src[80];
    __shared__ uint32_t s_pend, s_drop, s_unsup, s_full, s_ok, s_claim, s_abort, s_ncold;
    __shared__ __attribute__((aligned(16))) unsigned long long s_htab[kExHotTab];
    __shared__ unsigned long long s_hcb[kExHot];
    __shared__ uint32_t s_hmax[kExHot];
    const uint32_t tid = threadIdx.x, blk = blockIdx.x;
    if (tid == 0) { s_pend = 0; s_drop = 0; s_unsup = 0; s_full = 0; s_ok = 0; s_claim = 0; s_ncold = 0; s_abort = dict_aborted(a.D); }
    for (uint32_t i = tid; i < kExHotTab; i += kXThreads) s_htab[i] = a.hot_tab[i];
    for (uint32_t i = tid; i < kExHot; i += kXThreads) { s_hcb[i] = 0; s_hmax[i] = 0; }
    const ExHotLds H{s_htab, s_hcb, s_hmax};
    __syncthreads();
    if (s_abort) {  // the batch overflowed the dictionary: re-run after the table grows
        if (tid == 0) a.pend_cnt[blk] = 0;
        return;
    }
    stage_plan<MODE>(a.kp, s_src);
    const uint32_t K = a.kp.K;
    const uint64_t beg = (uint64_t)blk * kXChunk;
    const uint64_t end = min(a.n, beg + kXChunk);
    uint32_t n_ok = 0;
    if constexpr (KIND == IN_HDR) {
        // Two-stage software pipeline (as Count-Min's K1): iteration k parses packet
        // k+1 and issues its home-slot probe (and the record prefetch of packet k+2),
        // then consumes packet k, whose probe was issued one iteration earlier.
        uint4 hv[4];
        uint32_t hsz;
        auto load_hdr = [&](uint64_t q) {
            const uint64_t pc = min(q, end - 1);
            const uint4 *r = reinterpret_cast<const uint4 *>(a.x.in.hdr + pc * 16);
#pragma unroll
            for (int i = 0; i < 4; i++) hv[i] = r[i];
            hsz = a.x.in.sizes[pc];
        };
        auto stage_b = [&](uint64_t q, bool &okq, uint32_t (&kwq)[GNS_KWMAX], uint32_t &slotq, uint4 (&r4q)[4],
                           uint32_t &szq) {
            okq = q < end;
            uint32_t cw[16];
#pragma unroll
            for (int i = 0; i < 4; i++) { cw[4 * i] = hv[i].x; cw[4 * i + 1] = hv[i].y; cw[4 * i + 2] = hv[i].z; cw[4 * i + 3] = hv[i].w; }
            szq = hsz;
            load_hdr(q + kXThreads);
#pragma unroll
            for (int i = 0; i < GNS_KWMAX; i++) kwq[i] = 0;
            if (okq) {
                uint32_t tw[10];
                int st = parse_record_fast(cw, szq, true, tw);
                if (st == PARSE_OK) st = ex_key_tw<KIND, MODE>(a.x, K, s_src, q, tw, kwq);
                if (st != PARSE_OK) {
                    atomicAdd(st == PARSE_DROP ? &s_drop : &s_unsup, 1u);
                    okq = false;
                }
            }
            slotq = mm3_n<GNS_KWMAX>(kwq, K, a.D.seed) & a.D.mask;
            if (okq) ex_probe_issue(a.D, slotq, r4q);
        };
        load_hdr(beg + tid);
        bool okc;
        uint32_t kwc[GNS_KWMAX], slotc, szc;
        uint4 r4c[4];
        stage_b(beg + tid, okc, kwc, slotc, r4c, szc);
        for (uint64_t p0 = beg; p0 < end; p0 += kXThreads) {  // wave-uniform trip count
            bool okn = false;
            uint32_t kwn[GNS_KWMAX], slotn = 0, szn = 0;
            uint4 r4n[4];
            if (p0 + kXThreads < end) stage_b(p0 + kXThreads + tid, okn, kwn, slotn, r4n, szn);
            uint32_t park;
            const uint64_t w = ex_consume(a, p0 + tid, beg, okc, kwc, K, slotc, r4c, szc, &s_full, &s_claim, n_ok, H, park);
            ex_emit_park(a, beg, p0 + tid, w, park, &s_ncold, &s_pend);
            okc = okn; slotc = slotn; szc = szn;
#pragma unroll
            for (int i = 0; i < GNS_KWMAX; i++) kwc[i] = kwn[i];
#pragma unroll
            for (int i = 0; i < 4; i++) r4c[i] = r4n[i];
        }
    } else {
        for (uint64_t p0 = beg; p0 < end; p0 += kXThreads) {  // wave-uniform trip count
            const uint64_t p = p0 + tid;
            bool ok = p < end;
            uint32_t kw[GNS_KWMAX];
            const uint32_t sz = ok ? a.x.in.sizes[p] : 0u;
            if (ok) {
                const int st = ex_key<KIND, MODE>(a.x, K, s_src, p, kw);
                if (st != PARSE_OK) {
                    atomicAdd(st == PARSE_DROP ? &s_drop : &s_unsup, 1u);
                    ok = false;
                }
            }
            uint4 r4[4];
            uint32_t slot0 = 0;
            if (ok) {
                slot0 = mm3_n<GNS_KWMAX>(kw, K, a.D.seed) & a.D.mask;
                ex_probe_issue(a.D, slot0, r4);
            }
            uint32_t park;
            const uint64_t w = ex_consume(a, p, beg, ok, kw, K, slot0, r4, sz, &s_full, &s_claim, n_ok, H, park);
            ex_emit_park(a, beg, p, w, park, &s_ncold, &s_pend);
        }
    }
    atomicAdd(&s_ok, n_ok);
    __syncthreads();
    for (uint32_t i = tid; i < kExHot; i += kXThreads) {
        ExHotPart hp;
        hp.cb = s_hcb[i]; hp.maxp = s_hmax[i]; hp.pad = 0;
        a.hpart[(uint64_t)i * a.nblk + blk] = hp;
    }
    if (tid == 0) {
        a.pend_cnt[blk] = s_pend;
        a.ccnt[blk] = s_ncold;
        if (s_pend) atomicAdd(a.pend_total, s_pend);
        if (s_ok) atomicAdd(&a.stats[0], (unsigned long long)s_ok);
        if (s_drop) atomicAdd(&a.stats[1], (unsigned long long)s_drop);
        if (s_unsup) atomicAdd(&a.stats[2], (unsigned long long)s_unsup);
        if (s_full) atomicAdd(&a.stats[3], (unsigned long long)s_full);
        dict_flush_claims(a.D, s_claim, &a.stats[3]);
    }
}

struct ExResolveArgs {
    ExArgs x;
    const uint64_t *pend_in;
    const uint32_t *cnt_in;
    uint64_t *pend_out;
    uint32_t *cnt_out, *total_out;
};

template <int KIND, int MODE>
__global__ __launch_bounds__(kXThreads) void k_ex_resolve(ExResolveArgs r) {
    __shared__ uint8_t s_src[80];
    __shared__ uint32_t s_cnt, s_full, s_claim, s_abort;
    __shared__ __attribute__((aligned(16))) unsigned long long s_htab[kExHotTab];
    __shared__ unsigned long long s_hcb[kExHot];
    __shared__ uint32_t s_hmax[kExHot];
    const ExArgs &a = r.x;
    const uint32_t tid = threadIdx.x, blk = blockIdx.x;
    const uint32_t cnt = r.cnt_in[blk];
    if (cnt == 0) {  // block-uniform
        if (tid == 0) r.cnt_out[blk] = 0;
        return;
    }
    if (tid == 0) { s_cnt = 0; s_full = 0; s_claim = 0; s_abort = dict_aborted(a.D); }
    for (uint32_t j = tid; j < kExHotTab; j += kXThreads) s_htab[j] = a.hot_tab[j];
    for (uint32_t j = tid; j < kExHot; j += kXThreads) { s_hcb[j] = 0; s_hmax[j] = 0; }
    __syncthreads();
    if (s_abort) {
        if (tid == 0) r.cnt_out[blk] = 0;
        return;
    }
    stage_plan<MODE>(a.kp, s_src);
    const uint64_t beg = (uint64_t)blk * kXChunk;
    for (uint32_t i = tid; i < cnt; i += kXThreads) {
        const uint64_t v = r.pend_in[beg + i];
        const uint64_t p = beg + (v >> 50);
        uint32_t kw[GNS_KWMAX];
        (void)ex_key<KIND, MODE>(a.x, a.kp.K, s_src, p, kw);
        uint32_t out;
        const int res = dict_find_or_claim(a.D, kw, (uint32_t)(v & 0xFFFFFFFFFull), a.epoch, &out);
        if (res == DICT_CLAIMED) atomicAdd(&s_claim, 1u);
        if (res == DICT_FOUND || res == DICT_CLAIMED) {  // X1 wrote the word with none_key: fill in the flow field
            // a designated flow displaced from its home slot: into the block's partials
            // (its word is marked hot_key and skipped by P), as X1 does at the home slot
            const int h = res == DICT_FOUND ? exh_lookup(s_htab, out) : -1;
            if (h >= 0) {
                atomicAdd(&s_hcb[h], (unsigned long long)a.x.in.sizes[p] << kHotCntBits | 1ull);
                atomicMax(&s_hmax[h], (uint32_t)(p - beg));
                out = a.hot_key;
            }
            const uint32_t sh = a.ib + a.sb;
            const uint64_t wq = beg + ((v >> 36) & 0x3FFFu);
            a.sk[wq] = (a.sk[wq] & ((1ull << sh) - 1ull)) | (uint64_t)out << sh;
        }
        else if (res == DICT_PENDING) r.pend_out[beg + atomicAdd(&s_cnt, 1u)] = (v & ~0xFFFFFFFFFull) | out;
        else atomicAdd(&s_full, 1u);
    }
    __syncthreads();
    for (uint32_t j = tid; j < kExHot; j += kXThreads)
        if (s_hcb[j]) {  // X1 wrote this block's partials before this launch
            ExHotPart *hp = a.hpart + (uint64_t)j * a.nblk + blk;
            atomicAdd(&hp->cb, s_hcb[j]);
            atomicMax(&hp->maxp, s_hmax[j]);
        }
    if (tid == 0) {
        r.cnt_out[blk] = s_cnt;
        if (s_cnt) atomicAdd(r.total_out, s_cnt);
        if (s_full) atomicAdd(&a.stats[3], (unsigned long long)s_full);
        dict_flush_claims(a.D, s_claim, &a.stats[3]);
    }
}

// per-flow state, one array per field: first = stream index of the first packet (~0: none
// yet), last = stream index of the last packet + 1 (0: none), start / end = StartTime /
// EndTime in ns.  (One 64-byte record per flow measured slower: a run's two counter
// atomics then hit one line.)
struct FlowState {
    unsigned long long *pkts, *bytes, *first, *last;
    long long *start, *end;
};

extern "C" __device__ unsigned long long __ockl_wfred_add_u64(unsigned long long);
extern "C" __device__ unsigned __ockl_wfred_min_u32(unsigned);
extern "C" __device__ unsigned __ockl_wfred_max_u32(unsigned);
extern "C" __device__ unsigned __ockl_wfred_add_u32(unsigned);
// (__ockl_wfscan_add_u32: declared by gns_scan.cuh)

// H: the per-block partials of each designated flow -> its flow state (one
// workgroup per hot slot; the only writer of these flows until P4, which merges
// the flow's packets that were parked in X1).  first stays: a designated flow
// had packets before this batch.
template <bool LIST>
__global__ __launch_bounds__(256) void k_ex_hot_reduce(const ExHotPart *hpart, uint32_t nblk, const uint32_t *hot_ids,
                                                       uint64_t pkt_base, FlowState f, uint32_t *touch, uint32_t *tcnt) {
    __shared__ unsigned long long s_by[4];
    __shared__ uint32_t s_c[4], s_mx[4];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t id = hot_ids[slot];
    if (id == GNS_ID_NONE) return;  // block-uniform
    uint32_t c = 0, mx = 0;
    unsigned long long by = 0;
    for (uint32_t b = tid; b < nblk; b += 256) {
        const ExHotPart hp = hpart[(uint64_t)slot * nblk + b];
        if (hp.cb) {
            c += (uint32_t)(hp.cb & ((1u << kHotCntBits) - 1u));
            by += hp.cb >> kHotCntBits;
            mx = max(mx, b * kXChunk + hp.maxp);
        }
    }
    c = __ockl_wfred_add_u32(c);
    by = __ockl_wfred_add_u64(by);
    mx = __ockl_wfred_max_u32(mx);
    if (lane == 0) { s_c[wave] = c; s_by[wave] = by; s_mx[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) { c += s_c[w]; by += s_by[w]; mx = max(mx, s_mx[w]); }
        if (c) {
            f.pkts[id] += c;
            f.bytes[id] += by;
            f.last[id] = max(f.last[id], pkt_base + mx + 1);
            // H lists the designated flows it updated; P lists a flow only on its first merge
            // of the batch (last <= pkt_base), and H has already moved `last` past pkt_base
            // here, so parked packets of a designated flow never add a second entry
            if constexpr (LIST) touch[atomicAdd(tcnt, 1u)] = id;
        }
    }
}

// P: the tail words go to kPBins bins of consecutive flow ids (order-free: no
// stable partition is needed, the merge is add / min / max), then one
// workgroup per bin aggregates its words in an LDS hash table and merges each
// flow once.  Every flow id lies in exactly one bin, so the merge needs no
// global atomics.
//   P1 k_ex_phist     per X1 region: bin histogram  -> ph[blk][bin]
//   P2 k_ex_pscan_*   exclusive offsets of every (region, bin) in bin-major order
//   P3 k_ex_pscatter  per region, sub-passes of kPSub words staged bin by bin in
//                     LDS and copied out as runs
//   P4 k_ex_pagg      per bin: LDS hash (flow id -> count, bytes, min / max
//                     index), flushed into the flow state
constexpr uint32_t kPBinBits = 9;
constexpr uint32_t kPBins = 1u << kPBinBits;
constexpr uint32_t kPGroup = 64;  // regions per P2 group

__global__ __launch_bounds__(256) void k_ex_phist(const uint64_t *in, const uint32_t *ccnt, uint32_t ks,
                                                  uint32_t pshift, uint32_t none_key, uint32_t *ph) {
    __shared__ uint32_t h[kPBins];
    const uint32_t blk = blockIdx.x, n = ccnt[blk];
    for (uint32_t i = threadIdx.x; i < kPBins; i += 256) h[i] = 0;
    __syncthreads();
    const uint64_t *w = in + (uint64_t)blk * kXChunk;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t id = (uint32_t)(w[i] >> ks);
        if (id < none_key) atomicAdd(&h[id >> pshift], 1u);  // (a resolved designated flow's word is skipped)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kPBins; i += 256) ph[(uint64_t)blk * kPBins + i] = h[i];
}
// per group of kPGroup regions: bin sums
__global__ __launch_bounds__(kPBins) void k_ex_pscan_a(const uint32_t *ph, uint32_t nblk, uint32_t *gs) {
    const uint32_t g = blockIdx.x, b = threadIdx.x;
    const uint32_t r1 = min(nblk, (g + 1) * kPGroup);
    uint32_t sum = 0;
    for (uint32_t r = g * kPGroup; r < r1; r++) sum += ph[(uint64_t)r * kPBins + b];
    gs[(uint64_t)g * kPBins + b] = sum;
}
// one workgroup: per bin, exclusive offsets of the groups; bin starts (pb[kPBins] = total)
__global__ __launch_bounds__(kPBins) void k_ex_pscan_b(uint32_t *gs, uint32_t ng, uint32_t *pb) {
    __shared__ uint32_t s_w[kPBins / 64];
    const uint32_t b = threadIdx.x, lane = b & 63u, wave = b >> 6;
    uint32_t run = 0;
    for (uint32_t g0 = 0; g0 < ng; g0 += 8) {  // 8 independent loads in flight, then the prefix
        uint32_t x[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) x[j] = g0 + j < ng ? gs[(uint64_t)(g0 + j) * kPBins + b] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            if (g0 + j < ng) gs[(uint64_t)(g0 + j) * kPBins + b] = run;
            run += x[j];
        }
    }
    const uint32_t inc = __ockl_wfscan_add_u32(run, true);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; w++) base += s_w[w];
    const uint32_t start = base + inc - run;
    pb[b] = start;
    if (b == kPBins - 1) pb[kPBins] = base + inc;
    for (uint32_t g0 = 0; g0 < ng; g0 += 8) {
        uint32_t x[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) x[j] = g0 + j < ng ? gs[(uint64_t)(g0 + j) * kPBins + b] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (g0 + j < ng) gs[(uint64_t)(g0 + j) * kPBins + b] = x[j] + start;
    }
}
// per group: the regions' offsets, in place over the histogram
__global__ __launch_bounds__(kPBins) void k_ex_pscan_c(uint32_t *ph, uint32_t nblk, const uint32_t *gs) {
    const uint32_t g = blockIdx.x, b = threadIdx.x;
    const uint32_t r1 = min(nblk, (g + 1) * kPGroup);
    uint32_t run = gs[(uint64_t)g * kPBins + b];
    for (uint32_t r = g * kPGroup; r < r1; r++) {
        const uint32_t x = ph[(uint64_t)r * kPBins + b];
        ph[(uint64_t)r * kPBins + b] = run;
        run += x;
    }
}

constexpr uint32_t kPSub = 4096;  // words per P3 sub-pass
constexpr uint32_t kPItems = kPSub / kPBins;
__global__ __launch_bounds__(kPBins) void k_ex_pscatter(const uint64_t *in, const uint32_t *ccnt, const uint32_t *po,
                                                        uint32_t ks, uint32_t pshift, uint32_t none_key, uint64_t *out) {
    __shared__ uint64_t stage[kPSub];
    __shared__ uint16_t sbin[kPSub];
    __shared__ uint32_t cnt[kPBins], lstart[kPBins], goff[kPBins], dummy[kPBins], s_w[kPBins / 64];
    const uint32_t blk = xcd_block(blockIdx.x, gridDim.x);  // adjacent regions on one XCD (gns_xcd.cuh)
    const uint32_t n = ccnt[blk], tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (n == 0) return;  // block-uniform
    const uint64_t *src = in + (uint64_t)blk * kXChunk;
    goff[tid] = po[(uint64_t)blk * kPBins + tid];
    cnt[tid] = 0;
    __syncthreads();
    for (uint32_t sp = 0; sp < n; sp += kPSub) {
        uint64_t w[kPItems];
        uint32_t bn[kPItems], rk[kPItems];
#pragma unroll
        for (uint32_t j = 0; j < kPItems; j++) {
            const uint32_t i = sp + j * kPBins + tid;
            w[j] = i < n ? src[i] : 0ull;
            const uint32_t id = (uint32_t)(w[j] >> ks);
            bn[j] = i < n && id < none_key ? id >> pshift : 0xFFFFu;
        }
        // ranks (any order): every lane adds, a lane without a word adds 0 to its own word
#pragma unroll
        for (uint32_t j = 0; j < kPItems; j++) {
            uint32_t *ad = bn[j] != 0xFFFFu ? &cnt[bn[j]] : &dummy[tid];
            rk[j] = atomicAdd(ad, bn[j] != 0xFFFFu ? 1u : 0u);
        }
        __syncthreads();
        const uint32_t c = cnt[tid];
        const uint32_t inc = __ockl_wfscan_add_u32(c, true);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t v = 0; v < wave; v++) base += s_w[v];
        lstart[tid] = base + inc - c;
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kPItems; j++)
            if (bn[j] != 0xFFFFu) {
                const uint32_t pos = lstart[bn[j]] + rk[j];
                stage[pos] = w[j];
                sbin[pos] = (uint16_t)bn[j];
            }
        __syncthreads();
        uint32_t m = 0;  // words staged in this sub-pass (designated flows' words are not)
        for (uint32_t v = 0; v < kPBins / 64; v++) m += s_w[v];
        for (uint32_t i = tid; i < m; i += kPBins) {
            const uint32_t bb = sbin[i];
            out[goff[bb] + (i - lstart[bb])] = stage[i];
        }
        __syncthreads();
        goff[tid] += c;
        cnt[tid] = 0;
        __syncthreads();
    }
}

// P4: one workgroup per bin, two per CU.  Words in chunks of kAggChunk; before a
// chunk the table is flushed if it could overflow (a bin with more distinct flows
// than the table merges in several rounds; each flow's partial results add up).
// A flow holding >= 6 of a wave's words (a heavy tail flow) has them folded into
// one update (up to GNS_AGG_FOLD such flows per wave and chunk).
constexpr uint32_t kAggThreads = 1024;
constexpr uint32_t kAggChunk = kAggThreads;
#ifndef GNS_AGG_DEPTH
#define GNS_AGG_DEPTH 1
#endif
constexpr uint32_t kAggDepth = GNS_AGG_DEPTH;  // chunks of words in flight
#ifndef GNS_AGG_CAP
#define GNS_AGG_CAP 3072
#endif
#ifndef GNS_AGG_FOLD
#define GNS_AGG_FOLD 4
#endif
constexpr uint64_t kExListSlots = 1ull << 23;  // T/D read the touched list above this many slots
constexpr uint32_t kAggCap = GNS_AGG_CAP;  // 24 B per entry: 72 KB
constexpr int kAggMinBlocks = kAggCap * 24 <= 78 * 1024 ? 2 : 1;
static_assert(kAggCap > kAggChunk, "a chunk fits an empty table");
// Touched-flow list (T and D read it instead of scanning the table): a flow is
// appended when its first merge of the batch lands (its last index is then still
// from an earlier batch), so each flow appears once.  One global add per flush
// for the whole workgroup's appends (the counter is shared by every workgroup).

template <bool LIST>
__device__ __forceinline__ void pagg_flush(uint32_t *key, uint32_t *cn, uint32_t *mn, uint32_t *mx,
                                           unsigned long long *by, uint64_t pkt_base, FlowState f, uint32_t *touch,
                                           uint32_t *tcnt) {
    // every entry's four state words are loaded before any is merged (all in flight together)
    constexpr uint32_t kPer = (kAggCap + kAggThreads - 1) / kAggThreads;
    uint32_t id[kPer];
    unsigned long long pk[kPer], bt[kPer], ls[kPer], fs[kPer];
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t e = threadIdx.x + j * kAggThreads;
        id[j] = e < kAggCap ? key[e] : GNS_ID_NONE;
        if (id[j] != GNS_ID_NONE) { pk[j] = f.pkts[id[j]]; bt[j] = f.bytes[id[j]]; ls[j] = f.last[id[j]]; fs[j] = f.first[id[j]]; }
    }
    if constexpr (LIST) {  // the touched-flow list (large tables only: the scan variant compiles without it)
        __shared__ uint32_t s_tw[kAggThreads / 64], s_tbase;
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) c += (id[j] != GNS_ID_NONE && ls[j] <= pkt_base) ? 1u : 0u;
        const uint32_t inc = __ockl_wfscan_add_u32(c, true);
        if (lane == 63) s_tw[wave] = inc;
        __syncthreads();
        const uint32_t x = lane < kAggThreads / 64 ? s_tw[lane] : 0u;
        const uint32_t winc = __ockl_wfscan_add_u32(x, true);
        const uint32_t tot = __shfl(winc, 63);  // (all lanes active)
        if (threadIdx.x == 0) s_tbase = atomicAdd(tcnt, tot);
        __syncthreads();
        uint32_t pos = s_tbase + __shfl(winc - x, (int)wave) + inc - c;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
            if (id[j] != GNS_ID_NONE && ls[j] <= pkt_base) touch[pos++] = id[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t e = threadIdx.x + j * kAggThreads;
        if (id[j] == GNS_ID_NONE) continue;
        f.pkts[id[j]] = pk[j] + cn[e];
        f.bytes[id[j]] = bt[j] + by[e];
        f.last[id[j]] = max(ls[j], pkt_base + mx[e] + 1);
        if (fs[j] >= pkt_base) f.first[id[j]] = min(fs[j], pkt_base + mn[e]);  // no packet before this batch
        key[e] = GNS_ID_NONE; cn[e] = 0; mn[e] = ~0u; mx[e] = 0; by[e] = 0;
    }
}
// Table slot of a flow: buckets of 4 keys read with one 16-byte LDS load; keys
// fill a bucket's slots in order and spill to the next bucket only when it is
// full, so a bucket with an empty slot and no match ends the search (a linear
// probe of single keys measured long dependent chains at 2/3 load).
constexpr uint32_t kAggBuckets = kAggCap / 4;
static_assert(kAggCap % 4 == 0, "whole buckets");
__device__ __forceinline__ uint32_t pagg_slot(uint32_t *key, uint32_t id, uint32_t *s_n) {
    uint32_t b = (uint32_t)(((uint64_t)(id * 0x9E3779B1u) * kAggBuckets) >> 32);
    for (;;) {
        const uint4 k4 = reinterpret_cast<const uint4 *>(key)[b];
        if (k4.x == id) return 4 * b;
        if (k4.y == id) return 4 * b + 1;
        if (k4.z == id) return 4 * b + 2;
        if (k4.w == id) return 4 * b + 3;
        const uint32_t e = k4.x == GNS_ID_NONE ? 0u : k4.y == GNS_ID_NONE ? 1u : k4.z == GNS_ID_NONE ? 2u
                         : k4.w == GNS_ID_NONE ? 3u : 4u;
        if (e == 4u) {  // full: the key, if present, is further along
            b = b + 1 == kAggBuckets ? 0u : b + 1;
            continue;
        }
        const uint32_t old = atomicCAS(&key[4 * b + e], GNS_ID_NONE, id);
        if (old == GNS_ID_NONE) { atomicAdd(s_n, 1u); return 4 * b + e; }
        if (old == id) return 4 * b + e;
        // another flow took that slot: read the bucket again
    }
}
template <bool LIST>
__global__ __launch_bounds__(kAggThreads, kAggMinBlocks) void k_ex_pagg(const uint64_t *in, const uint32_t *pb, uint32_t sb,
                                                            uint32_t ib, const uint32_t *sizes, uint64_t pkt_base,
                                                            FlowState f, uint32_t *touch, uint32_t *tcnt) {
    __shared__ __attribute__((aligned(16))) uint32_t key[kAggCap];
    __shared__ uint32_t cn[kAggCap], mn[kAggCap], mx[kAggCap];
    __shared__ unsigned long long by[kAggCap];
    __shared__ uint32_t s_n;
    const uint32_t bin = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t beg = pb[bin], end = pb[bin + 1];
    if (beg == end) return;  // block-uniform
    for (uint32_t e = tid; e < kAggCap; e += kAggThreads) { key[e] = GNS_ID_NONE; cn[e] = 0; mn[e] = ~0u; mx[e] = 0; by[e] = 0; }
    if (tid == 0) s_n = 0;
    const uint32_t ks = sb + ib, esc = (1u << sb) - 1u;
    const uint64_t imask = (1ull << ib) - 1ull;
    // the words of the next kAggDepth chunks are in flight (P4 is latency-bound on them)
    uint64_t wq[kAggDepth];
#pragma unroll
    for (uint32_t j = 0; j < kAggDepth; j++) {
        const uint32_t i = beg + j * kAggChunk + tid;
        wq[j] = i < end ? in[i] : ~0ull;
    }
    __syncthreads();
    for (uint32_t c0 = beg; c0 < end; c0 += kAggChunk) {  // block-uniform trip count
        if (s_n > kAggCap - kAggChunk) {  // block-uniform (read after the barrier)
            pagg_flush<LIST>(key, cn, mn, mx, by, pkt_base, f, touch, tcnt);
            __syncthreads();
            if (tid == 0) s_n = 0;
            __syncthreads();
        }
        const uint64_t w = wq[0];
#pragma unroll
        for (uint32_t j = 0; j + 1 < kAggDepth; j++) wq[j] = wq[j + 1];
        {
            const uint32_t i = c0 + kAggDepth * kAggChunk + tid;
            wq[kAggDepth - 1] = i < end ? in[i] : ~0ull;
        }
        bool v = w != ~0ull;
        const uint32_t id = v ? (uint32_t)(w >> ks) : GNS_ID_NONE;
        const uint32_t idx = (uint32_t)((w >> sb) & imask);
        uint32_t sz = (uint32_t)w & esc;
        if (v && sz == esc) sz = sizes[idx];  // lengths too large for the word's field (rare)
        // heavy flows holding many of the wave's words: one folded update each
        // (same-address LDS atomics serialize lane by lane)
#pragma unroll 1
        for (int fold = 0; fold < GNS_AGG_FOLD; fold++) {
            const uint64_t vm = __ballot(v);
            if (!vm) break;  // wave-uniform
            const uint32_t id0 = __shfl(id, (int)(__ffsll((long long)vm) - 1));
            const bool in_m = v && id == id0;
            const uint64_t m = __ballot(in_m);
            if (__popcll(m) < 6) break;  // wave-uniform
            const unsigned long long tb = __ockl_wfred_add_u64(in_m ? (unsigned long long)sz : 0ull);
            const uint32_t tmn = __ockl_wfred_min_u32(in_m ? idx : ~0u);
            const uint32_t tmx = __ockl_wfred_max_u32(in_m ? idx : 0u);
            if (lane == (uint32_t)__ffsll((long long)m) - 1u) {
                const uint32_t h = pagg_slot(key, id0, &s_n);
                atomicAdd(&cn[h], (uint32_t)__popcll(m));
                atomicAdd(&by[h], tb);
                atomicMin(&mn[h], tmn);
                atomicMax(&mx[h], tmx);
            }
            v = v && !in_m;
        }
        if (v) {
            const uint32_t h = pagg_slot(key, id, &s_n);
            atomicAdd(&cn[h], 1u);
            atomicAdd(&by[h], (unsigned long long)sz);
            atomicMin(&mn[h], idx);
            atomicMax(&mx[h], idx);
        }
        __syncthreads();
    }
    pagg_flush<LIST>(key, cn, mn, mx, by, pkt_base, f, touch, tcnt);
}

// T: StartTime / EndTime from the merged stream indices of the flows this batch
// touched (task.go:137,141-142).
__global__ __launch_bounds__(256) void k_ex_times(FlowState f, uint64_t slots, uint64_t pkt_base, uint64_t n,
                                                  const int64_t *ts) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const unsigned long long l = f.last[s], fs = f.first[s];
    if (l > pkt_base && l <= pkt_base + n) f.end[s] = ts[l - 1 - pkt_base];
    if (fs >= pkt_base && fs < pkt_base + n) f.start[s] = ts[fs - pkt_base];
}

// D: designate the next batch's heavy flows: the flows in the largest 1/8-octave
// bands of the packet count that together hold at most kExHot flows.
__device__ __forceinline__ uint32_t exh_key(unsigned long long p) {
    if (p < 8) return 0;
    const uint32_t lz = 63u - (uint32_t)__clzll((long long)p);
    return lz * 8u + (uint32_t)((p >> (lz - 3)) & 7u);
}
__global__ __launch_bounds__(256) void k_exh_hist(const unsigned long long *pkts, uint64_t slots, uint32_t *hist) {
    __shared__ uint32_t h[512];
    for (uint32_t i = threadIdx.x; i < 512; i += 256) h[i] = 0;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {
        const uint32_t k = exh_key(pkts[s]);
        if (k >= kExHotMinKey) atomicAdd(&h[k], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 512; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}
// threshold = the smallest key whose suffix count (flows with a key >= it) is <= kExHot
__global__ __launch_bounds__(512) void k_exh_pick(const uint32_t *hist, uint32_t *thr) {
    __shared__ uint32_t s_w[8];
    __shared__ uint32_t s_t;
    const uint32_t k = threadIdx.x, lane = k & 63u, wave = k >> 6;
    if (k == 0) s_t = 512;
    // suffix sums: scan over the reversed keys
    const uint32_t r = 511u - k;  // thread k holds key r
    const uint32_t v = r >= kExHotMinKey ? hist[r] : 0u;
    const uint32_t inc = __ockl_wfscan_add_u32(v, true);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; w++) base += s_w[w];
    const uint32_t suffix = base + inc;  // flows with a key >= r
    if (r >= kExHotMinKey && suffix <= kExHot) atomicMin(&s_t, r);
    __syncthreads();
    if (k == 0) *thr = s_t;
}
__global__ __launch_bounds__(256) void k_exh_collect(const unsigned long long *pkts, uint64_t slots,
                                                     const uint32_t *thr, uint32_t *cnt, uint32_t *hot_ids) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const uint32_t k = exh_key(pkts[s]);
    if (k >= *thr && k >= kExHotMinKey) {
        const uint32_t q = atomicAdd(cnt, 1u);
        if (q < kExHot) hot_ids[q] = (uint32_t)s;
    }
}
// T and D over the batch's touched-flow list instead of every slot: tables above
// kExListSlots (a table that grew with the period), where a scan would cost more
// than the batch.  The list's random gathers cost more than the scan below that.
__global__ __launch_bounds__(256) void k_ex_times_list(FlowState f, const uint32_t *touch, const uint32_t *tcnt,
                                                  uint64_t slots, uint64_t pkt_base, uint64_t n, const int64_t *ts) {
    const uint64_t nt = *tcnt;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nt; i += (uint64_t)gridDim.x * 256) {
        const uint32_t s = touch[i];
        const unsigned long long l = f.last[s], fs = f.first[s];
        if (l > pkt_base && l <= pkt_base + n) f.end[s] = ts[l - 1 - pkt_base];
        if (fs >= pkt_base && fs < pkt_base + n) f.start[s] = ts[fs - pkt_base];
    }
}

__global__ __launch_bounds__(256) void k_exh_hist_list(const unsigned long long *pkts, const uint32_t *touch,
                                                  const uint32_t *tcnt, uint64_t slots, uint32_t *hist) {
    __shared__ uint32_t h[512];
    for (uint32_t i = threadIdx.x; i < 512; i += 256) h[i] = 0;
    __syncthreads();
    const uint64_t nt = *tcnt;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nt; i += (uint64_t)gridDim.x * 256) {
        const uint32_t k = exh_key(pkts[touch[i]]);
        if (k >= kExHotMinKey) atomicAdd(&h[k], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 512; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}
__global__ __launch_bounds__(256) void k_exh_collect_list(const unsigned long long *pkts, const uint32_t *touch,
                                                     const uint32_t *tcnt, uint64_t slots, const uint32_t *thr,
                                                     uint32_t *cnt, uint32_t *hot_ids) {
    const uint64_t nt = *tcnt;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nt; i += (uint64_t)gridDim.x * 256) {
        const uint32_t s = touch[i];
        const uint32_t k = exh_key(pkts[s]);
        if (k >= *thr && k >= kExHotMinKey) {
            const uint32_t q = atomicAdd(cnt, 1u);
            if (q < kExHot) hot_ids[q] = s;
        }
    }
}
// the lookup table, heaviest flows first (64 at a time): a flow whose 4-entry group
// is full is simply not designated, and that should be one of the lightest
// (a heavy flow left in the tail would serialise its P4 bin)
__global__ __launch_bounds__(kExHot) void k_exh_table(uint32_t *hot_ids, const unsigned long long *pkts,
                                                      unsigned long long *hot_tab) {
    __shared__ unsigned long long t[kExHotTab];
    __shared__ unsigned long long s_p[kExHot];
    __shared__ uint32_t s_ord[kExHot];
    const uint32_t i = threadIdx.x;
    for (uint32_t j = i; j < kExHotTab; j += kExHot) t[j] = ~0ull;
    const uint32_t id = hot_ids[i];
    const unsigned long long p = id != GNS_ID_NONE ? pkts[id] : 0ull;
    s_p[i] = p;
    __syncthreads();
    uint32_t rank = 0;
    for (uint32_t j = 0; j < kExHot; j++) {
        const unsigned long long q = s_p[j];
        rank += (q > p || (q == p && j < i)) ? 1u : 0u;
    }
    s_ord[rank] = i;
    __syncthreads();
    for (uint32_t r0 = 0; r0 < kExHot; r0 += 64) {
        if (i < 64) {
            const uint32_t h = s_ord[r0 + i];
            const uint32_t hid = hot_ids[h];
            if (hid != GNS_ID_NONE) {
                const uint32_t g = exh_group(hid) * 4;
                bool in = false;
                for (uint32_t e = 0; e < 4 && !in; e++)
                    in = atomicCAS(&t[g + e], ~0ull, (unsigned long long)hid << 16 | h) == ~0ull;
                if (!in) hot_ids[h] = GNS_ID_NONE;
            }
        }
        __syncthreads();
    }
    for (uint32_t j = i; j < kExHotTab; j += kExHot) hot_tab[j] = t[j];
}

__global__ __launch_bounds__(256) void k_ex_query(const uint8_t *flows, uint32_t stride, uint64_t n, uint32_t K,
                                                  DictDev D, FlowState f, uint64_t *out) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    uint32_t kw[GNS_KWMAX];
    load_key_bytes<GNS_KWMAX>(flows + p * stride, K, false, kw);
    const uint32_t id = dict_lookup(D, kw);
    out[p] = id == GNS_ID_NONE ? 0ull : (uint64_t)(f.pkts[id] << 32 | f.bytes[id]);  // task.go:323
}

// occupied dictionary slots -> ids (snapshot)
__global__ __launch_bounds__(256) void k_ex_list(DictDev D, uint64_t slots, const unsigned long long *pkts,
                                                 uint32_t *ids, uint32_t *count) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool occ = s < slots && D.rec[s * D.RW] != 0u && pkts[s] != 0ull;
    const uint64_t m = __ballot(occ);
    if (m == 0) return;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (occ) ids[base + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)s;
}

// ids == NULL: row p is record p (a snapshot view's dense rows); start == NULL: key bytes only
// (a view's state arrays are dense already)
__global__ __launch_bounds__(256) void k_ex_gather(const uint32_t *ids, uint64_t n, DictDev D, FlowState f,
                                                   uint8_t *keys, long long *start, long long *end,
                                                   unsigned long long *pkts, unsigned long long *bytes) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t id = ids ? ids[p] : (uint32_t)p;
    uint32_t r[12];
    load_record(D, id, r);
    for (uint32_t j = 0; j < D.K; j++) keys[p * D.K + j] = (uint8_t)(r[1 + (j >> 2)] >> (8 * (j & 3)));
    if (start) { start[p] = f.start[id]; end[p] = f.end[id]; pkts[p] = f.pkts[id]; bytes[p] = f.bytes[id]; }
}

// ---------------------------------------------------------------------------
// Snapshot view (gns_ex_view_refresh): the selected flows -- occupied as k_ex_list
// has it, and touched after stream position `since` -- compacted in slot order into
// a dense table of the same layout (records at stride RW, one state array per
// field), so the query kernels below run on a view as on the live table.
//   V1 k_exv_count  per block of 256 slots: the number selected (wave ballots)
//   V2 k_tscan_*    exclusive offsets of the blocks, the total (gns_scan.cuh)
//   V3 k_exv_write  selected slot -> row = block offset + rank within the block
// The scan of gns_scan.cuh orders (bin, block) pairs bin-major; slot block i is
// given bin i / nb and block i % nb of kVBins bins, so that order is slot order
// and the scan's threads each own one bin.
// ---------------------------------------------------------------------------
constexpr uint32_t kVBins = 256;
__device__ __forceinline__ uint64_t exv_cell(uint32_t i, uint32_t nb) { return (uint64_t)(i % nb) * kVBins + i / nb; }
// (ExSelSince / ExSelAsOf: the row-selection policies, declared here for V1 / V3 and described
// with the query plane below)
struct ExSelSince {
    static constexpr bool kVersioned = false;
    unsigned long long since;
};
struct ExSelAsOf {
    static constexpr bool kVersioned = true;
    static constexpr bool kSigned = false;
    const uint32_t *written, *superseded;
    uint32_t s;
    __device__ __forceinline__ void test(uint64_t row, bool &seen, bool &live) const {
        const uint32_t a = written[row], b = superseded[row];
        seen = a <= s;
        live = seen && s < b;
    }
};
template <class SEL>
__device__ __forceinline__ bool exv_selected(const DictDev &D, const FlowState &f, uint64_t s, uint64_t slots,
                                             const SEL &sel) {
    if constexpr (SEL::kVersioned) {  // a history's as-of snapshot: the live rows, in log order
        bool seen = false, live = false;
        if (s < slots) sel.test(s, seen, live);
        return live;
    } else {
        return s < slots && D.rec[s * D.RW] != 0u && f.pkts[s] != 0ull && f.last[s] > sel.since;
    }
}
// grid = nb * kVBins blocks (>= the slot blocks; the cells past them count 0)
template <class SEL>
__device__ __forceinline__ void exv_count_block(const DictDev &D, uint64_t slots, const FlowState &f, const SEL &sl,
                                                uint32_t nb, uint32_t *cnt) {
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x;
    const bool sel = exv_selected(D, f, (uint64_t)blockIdx.x * 256 + tid, slots, sl);
    const uint64_t m = __ballot(sel);
    if ((tid & 63u) == 0) s_w[tid >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (tid == 0) cnt[exv_cell(blockIdx.x, nb)] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ __launch_bounds__(256) void k_exv_count(DictDev D, uint64_t slots, FlowState f, unsigned long long since,
                                                   uint32_t nb, uint32_t *cnt) {
    exv_count_block(D, slots, f, ExSelSince{since}, nb, cnt);
}
__global__ __launch_bounds__(256) void k_exhv_count(DictDev D, uint64_t slots, FlowState f, ExSelAsOf sel, uint32_t nb,
                                                    uint32_t *cnt) {
    exv_count_block(D, slots, f, sel, nb, cnt);
}
// V: the view's tables (cap rows each); a row past cap is not written (cap >= the claimed slots >= the rows)
template <class SEL>
__device__ __forceinline__ void exv_write_block(const DictDev &D, uint64_t slots, const FlowState &f, const SEL &sl,
                                                uint32_t nb, const uint32_t *off, const DictDev &V,
                                                const FlowState &vf, uint64_t cap) {
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t s = (uint64_t)blockIdx.x * 256 + tid;
    const bool sel = exv_selected(D, f, s, slots, sl);
    const uint64_t m = __ballot(sel);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!sel) return;
    uint64_t r = off[exv_cell(blockIdx.x, nb)] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) r += s_w[w];
    if (r >= cap) return;
    const uint4 *q = reinterpret_cast<const uint4 *>(D.rec + s * D.RW);
    uint4 *o = reinterpret_cast<uint4 *>(V.rec + r * D.RW);
    // {tag, key words} fill at most 11 words: the last quarter of a 16-word record holds nothing
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (4u * i < D.RW) o[i] = i < 3 ? q[i] : make_uint4(0, 0, 0, 0);
    vf.pkts[r] = f.pkts[s]; vf.bytes[r] = f.bytes[s]; vf.start[r] = f.start[s]; vf.end[r] = f.end[s];
}
__global__ __launch_bounds__(256) void k_exv_write(DictDev D, uint64_t slots, FlowState f, unsigned long long since,
                                                   uint32_t nb, const uint32_t *off, DictDev V, FlowState vf,
                                                   uint64_t cap) {
    exv_write_block(D, slots, f, ExSelSince{since}, nb, off, V, vf, cap);
}
__global__ __launch_bounds__(256) void k_exhv_write(DictDev D, uint64_t slots, FlowState f, ExSelAsOf sel, uint32_t nb,
                                                    const uint32_t *off, DictDev V, FlowState vf, uint64_t cap) {
    exv_write_block(D, slots, f, sel, nb, off, V, vf, cap);
}

// ---------------------------------------------------------------------------
// Query plane (gns_ex_aggregate / gns_ex_heavy_hitters): the Querier's questions
// (internal/query/querier.go) answered by scans of the resident table.
// ---------------------------------------------------------------------------
// Q: filtered aggregates.  A filter is equality on some key fields
// (appendAggregationFilters, querier.go:143-188).  The host turns it into one
// (mask, value) pair per little-endian key word of the record -- fields lie at
// the byte offsets of the handle's layout, aligned or not -- so a lane tests a
// filter with nkw AND / compare pairs on the key words it already holds.  One
// pass answers up to kQBatch filters: a lane loads its slot's tag, key words
// and state words once and tests every filter of the batch against them.  A
// filter some lane of the wave matches is reduced across the wave, merged into
// the workgroup's LDS partials, and leaves the CU as one set of global updates
// per workgroup and filter.  All of it is integer add / min / max: bit-exact in
// any order.  StartTime / EndTime are signed: they are reduced as unsigned
// words with the sign bit flipped, which keeps their order.
constexpr uint32_t kQBatch = 64;
#ifndef GNS_EXQ_NARROW
#define GNS_EXQ_NARROW 4
#endif
constexpr uint32_t kQNarrow = GNS_EXQ_NARROW;  // a batch of at most this many filters reduces each match across the wave
static_assert(kQBatch == 64, "the wide scan gives every lane of a wave one filter of the batch");
constexpr uint32_t kQAcc = 7;  // flows, packets, bytes, min start, max end, max packets, max bytes
constexpr unsigned long long kQSign = 1ull << 63;
struct ExQFilter {
    uint32_t m[GNS_KWMAX], v[GNS_KWMAX];  // match: (key word & m) == v for every key word
};
__host__ __device__ inline unsigned long long exq_acc_init(uint32_t j) { return j == 3 ? ~0ull : 0ull; }

extern "C" __device__ unsigned long long __ockl_wfred_min_u64(unsigned long long);
extern "C" __device__ unsigned long long __ockl_wfred_max_u64(unsigned long long);

// value of wave-uniform lane j
__device__ __forceinline__ unsigned long long exq_lane_u64(unsigned long long v, uint32_t j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
    return (unsigned long long)hi << 32 | lo;
}

// WIDE = false (a few filters): a filter some lane matches is reduced across the wave
// at once (six 64-bit wave reductions) into the workgroup's partials.
// WIDE = true: those reductions, per filter and table row of the wave, cost several
// times the filter tests themselves once a dozen filters match most flows.  So the wave
// is turned: lane q owns filter q of the batch (kQBatch = the wave width) and keeps its
// partials in registers for the whole scan; per row of 64 slots it gets the ballot of
// the lanes filter q matched, then walks the slots any filter matched -- their state
// words broadcast from the owning lane -- and merges those its ballot names.  One walk
// serves all 64 filters, and nothing is reduced before the scan ends.
//
// SEL is the row-selection policy of the scans (Q, HH1 / HH2, V1 / V3):
//   ExSelOcc    the live table and a view's rows: an occupied slot with packets
//   ExSelSince  V1 / V3 of a view: ExSelOcc and touched after a stream position
//   ExSelAsOf   a history's log as of snapshot s: a row is SEEN when written <= s and LIVE when
//               also s < superseded.  The version words are read first, and a wave none of
//               whose rows is seen loads neither records nor state: an interval outside the
//               query costs 8 B per row.  Sums and lists take the live rows, min / max the
//               seen ones (TraceFlow has no argMax).
// A scan kernel takes its policy as a trailing parameter pack: none for ExSelOcc, so the live
// table's and the views' instantiations keep their argument list.
struct ExSelOcc {
    static constexpr bool kVersioned = false;
    static constexpr bool kSigned = false;
};
// HH1 / HH2 of gns_ex_movers: ExSelOcc over a table whose counts are two's-complement changes.
// The value is the magnitude of the signed change (as u64: INT64_MIN has 2^63), taken when the
// change is not 0 and its sign matches dir (+1 increases, -1 decreases, 0 either).
struct ExSelSigned {
    static constexpr bool kVersioned = false;
    static constexpr bool kSigned = true;
    int dir;
};
__device__ __forceinline__ ExSelOcc exq_sel() { return ExSelOcc{}; }
__device__ __forceinline__ const ExSelAsOf &exq_sel(const ExSelAsOf &sel) { return sel; }
__device__ __forceinline__ const ExSelSigned &exq_sel(const ExSelSigned &sel) { return sel; }
template <class... SL> struct ExSelPick { using type = ExSelOcc; };
template <> struct ExSelPick<ExSelAsOf> { using type = ExSelAsOf; };
template <> struct ExSelPick<ExSelSigned> { using type = ExSelSigned; };
template <class... SL>
using ExSelOf = typename ExSelPick<SL...>::type;

template <bool WIDE, class... SL>
__global__ __launch_bounds__(256) void k_exq_aggregate(DictDev D, uint64_t slots, FlowState f,
                                                       const ExQFilter *__restrict__ flt, uint32_t nf,
                                                       unsigned long long *__restrict__ acc, SL... sl) {
    using SEL = ExSelOf<SL...>;
    [[maybe_unused]] const SEL sel = exq_sel(sl...);
    __shared__ unsigned long long s_a[kQBatch][kQAcc];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < nf * kQAcc; i += 256) s_a[i / kQAcc][i % kQAcc] = exq_acc_init(i % kQAcc);
    __syncthreads();
    const uint32_t nkw = (D.K + 3) >> 2;
    unsigned long long a_n = 0, a_pk = 0, a_by = 0, a_st = ~0ull, a_en = 0, a_mp = 0, a_mb = 0;  // WIDE: filter `lane`
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 < slots; s0 += (uint64_t)gridDim.x * 256) {  // block-uniform
        const uint64_t s = s0 + tid;
        uint32_t r[12];
        unsigned long long pk = 0, by = 0, st = ~0ull, en = 0;
        bool occ = false;
        [[maybe_unused]] bool cur = false;  // versioned: the row is live (occ: it is seen)
        if constexpr (SEL::kVersioned) {
            if (s < slots) sel.test(s, occ, cur);
            if (!__ballot(occ)) continue;  // wave-uniform: nothing seen, nothing loaded
            if (occ) {  // (a log row is a view's row: occupied, with packets)
                load_record(D, (uint32_t)s, r);
                pk = f.pkts[s]; by = f.bytes[s];
                st = (unsigned long long)f.start[s] ^ kQSign; en = (unsigned long long)f.end[s] ^ kQSign;
            }
        } else {
            if (s < slots) {
                load_record(D, (uint32_t)s, r);
                pk = f.pkts[s]; by = f.bytes[s];
                st = (unsigned long long)f.start[s] ^ kQSign; en = (unsigned long long)f.end[s] ^ kQSign;
                occ = r[0] != 0u && pk != 0ull;  // k_ex_list's occupancy rule
            }
            if (!__ballot(occ)) continue;  // wave-uniform
        }
        [[maybe_unused]] uint64_t curm = 0;  // versioned: the live rows of the wave
        if constexpr (SEL::kVersioned) curm = __ballot(cur);
        unsigned long long mine = 0;   // WIDE: the lanes filter `lane` matched
        bool any = false;
        for (uint32_t q = 0; q < nf; q++) {
            // the filter's words are wave-uniform: scalar loads, operands from scalar registers
            const ExQFilter *fq = flt + q;
            bool hit = occ;
#pragma unroll
            for (int i = 0; i < GNS_KWMAX; i++) {
                const uint32_t m = fq->m[i], v = fq->v[i];
                // every key word, open ones (m = v = 0) too: skipping them on a uniform branch
                // measured 30% slower than the two vector instructions it saves
                if ((uint32_t)i < nkw) hit = hit && ((r[1 + i] & m) == v);
            }
            const uint64_t hm = __ballot(hit);
            if constexpr (WIDE) {
                mine = lane == q ? hm : mine;
                any = any || hit;
            } else {
                if (!hm) continue;  // wave-uniform: every lane takes part in the reductions below
                bool add = hit;  // the row enters COUNT / SUM
                uint64_t am = hm;
                if constexpr (SEL::kVersioned) { add = hit && cur; am = hm & curm; }
                const unsigned long long tp = __ockl_wfred_add_u64(add ? pk : 0ull);
                const unsigned long long tb = __ockl_wfred_add_u64(add ? by : 0ull);
                const unsigned long long ts = __ockl_wfred_min_u64(hit ? st : ~0ull);
                const unsigned long long te = __ockl_wfred_max_u64(hit ? en : 0ull);
                const unsigned long long mp = __ockl_wfred_max_u64(hit ? pk : 0ull);
                const unsigned long long mb = __ockl_wfred_max_u64(hit ? by : 0ull);
                if (lane == 0) {
                    atomicAdd(&s_a[q][0], (unsigned long long)__popcll(am));
                    atomicAdd(&s_a[q][1], tp);
                    atomicAdd(&s_a[q][2], tb);
                    atomicMin(&s_a[q][3], ts);
                    atomicMax(&s_a[q][4], te);
                    atomicMax(&s_a[q][5], mp);
                    atomicMax(&s_a[q][6], mb);
                }
            }
        }
        if constexpr (WIDE) {
            uint64_t todo = __ballot(any);  // slots some filter matched (wave-uniform walk)
            while (todo) {
                const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
                todo &= todo - 1;
                const unsigned long long pj = exq_lane_u64(pk, j), bj = exq_lane_u64(by, j);
                const unsigned long long sj = exq_lane_u64(st, j), ej = exq_lane_u64(en, j);
                if (mine >> j & 1ull) {
                    bool add = true;  // versioned: only a live row enters COUNT / SUM
                    if constexpr (SEL::kVersioned) add = curm >> j & 1ull;
                    if (add) { a_n += 1; a_pk += pj; a_by += bj; }
                    a_st = min(a_st, sj); a_en = max(a_en, ej);
                    a_mp = max(a_mp, pj); a_mb = max(a_mb, bj);
                }
            }
        }
    }
    // something to merge: a row counted; versioned: a row seen (every row has packets, so
    // max(PacketCount) != 0), which a block may hold without the live row of the same key
    if constexpr (WIDE) {
        if (lane < nf && (SEL::kVersioned ? a_mp : a_n) != 0ull) {
            atomicAdd(&s_a[lane][0], a_n);
            atomicAdd(&s_a[lane][1], a_pk);
            atomicAdd(&s_a[lane][2], a_by);
            atomicMin(&s_a[lane][3], a_st);
            atomicMax(&s_a[lane][4], a_en);
            atomicMax(&s_a[lane][5], a_mp);
            atomicMax(&s_a[lane][6], a_mb);
        }
    }
    __syncthreads();
    if (tid < nf && s_a[tid][SEL::kVersioned ? 5 : 0] != 0ull) {
        unsigned long long *a = acc + (uint64_t)tid * kQAcc;
        atomicAdd(&a[0], s_a[tid][0]);
        atomicAdd(&a[1], s_a[tid][1]);
        atomicAdd(&a[2], s_a[tid][2]);
        atomicMin(&a[3], s_a[tid][3]);
        atomicMax(&a[4], s_a[tid][4]);
        atomicMax(&a[5], s_a[tid][5]);
        atomicMax(&a[6], s_a[tid][6]);
    }
}

// HH: the flows with value >= threshold in (value desc, key bytes asc) order, cut to
// `limit` rows.  Values are 64-bit and a row is a flow, so the 32-bit fingerprint
// list of gns_hh.hpp does not fit; as the hot-flow designation above (k_exh_*), a
// histogram over 1/8-octave bands of the value picks the lowest band the cut can
// reach, only the flows from that band up are compacted into rows (every flow
// below it is lighter than all of them, and equal values share a band, so ties at
// the cut are all candidates), and only those rows are ordered.
//   HH1 k_exq_hh_hist     band histogram of the qualifying flows (its sum = list length)
//   HH2 k_exq_hh_collect  rows {value, key words byte-swapped: word compare = byte compare}
//   HH3 rocprim::merge_sort of the rows by (value desc, key asc)
//   HH4 k_exq_hh_out      the first rows -> key bytes, values
constexpr uint32_t kQBands = 512;
__device__ __forceinline__ uint32_t exq_band(unsigned long long v) {
    if (v < 8) return 0;
    const uint32_t lz = 63u - (uint32_t)__clzll((long long)v);
    return lz * 8u + (uint32_t)((v >> (lz - 3)) & 7u);  // <= 63 * 8 + 7
}
struct ExHhRow {
    unsigned long long v;
    uint32_t k[GNS_KWMAX];
};
struct ExHhLess {
    __host__ __device__ bool operator()(const ExHhRow &a, const ExHhRow &b) const {
        if (a.v != b.v) return a.v > b.v;
#pragma unroll
        for (int i = 0; i < GNS_KWMAX; i++)
            if (a.k[i] != b.k[i]) return a.k[i] < b.k[i];
        return false;
    }
};
template <class SEL>
__device__ __forceinline__ bool exq_hh_take(const DictDev &D, const FlowState &f, uint64_t s, uint64_t slots, int metric,
                                            unsigned long long thr, unsigned long long &v, const SEL &sel) {
    if (s >= slots) return false;
    if constexpr (SEL::kVersioned) {  // the list holds the live rows; the others load no state
        bool seen, live;
        sel.test(s, seen, live);
        if (!live) return false;
        v = metric ? f.bytes[s] : f.pkts[s];
        return v >= thr;
    } else if constexpr (SEL::kSigned) {
        const unsigned long long pk = f.pkts[s];
        const unsigned long long c = metric ? f.bytes[s] : pk;
        const bool neg = (long long)c < 0;
        v = neg ? 0ull - c : c;  // |change|; thr >= 1 (the host's), so a change of 0 is not taken
        return D.rec[s * D.RW] != 0u && pk != 0ull && v >= thr && (sel.dir == 0 || (sel.dir < 0) == neg);
    } else {
        const unsigned long long pk = f.pkts[s];
        v = metric ? f.bytes[s] : pk;
        return D.rec[s * D.RW] != 0u && pk != 0ull && v >= thr;
    }
}
template <class... SL>
__global__ __launch_bounds__(256) void k_exq_hh_hist(DictDev D, uint64_t slots, FlowState f, int metric,
                                                     unsigned long long thr, uint32_t *hist, SL... sl) {
    [[maybe_unused]] const ExSelOf<SL...> sel = exq_sel(sl...);
    __shared__ uint32_t h[kQBands];
    for (uint32_t i = threadIdx.x; i < kQBands; i += 256) h[i] = 0;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256) {
        unsigned long long v;
        if (exq_hh_take(D, f, s, slots, metric, thr, v, sel)) atomicAdd(&h[exq_band(v)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kQBands; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}
template <class... SL>
__global__ __launch_bounds__(256) void k_exq_hh_collect(DictDev D, uint64_t slots, FlowState f, int metric,
                                                        unsigned long long thr, uint32_t band, ExHhRow *rows,
                                                        uint32_t *cnt, uint32_t cap, SL... sl) {
    [[maybe_unused]] const ExSelOf<SL...> sel = exq_sel(sl...);
    const uint32_t lane = __lane_id();
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256; s0 < slots; s0 += (uint64_t)gridDim.x * 256) {  // block-uniform
        const uint64_t s = s0 + threadIdx.x;
        unsigned long long v = 0;
        const bool take = exq_hh_take(D, f, s, slots, metric, thr, v, sel) && exq_band(v) >= band;
        const uint64_t m = __ballot(take);
        if (!m) continue;
        const int leader = __ffsll((unsigned long long)m) - 1;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(cnt, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        const uint32_t q = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (take && q < cap) {  // (cap = the histogram's count of these bands: never exceeded)
            uint32_t r[12];
            load_record(D, (uint32_t)s, r);
            ExHhRow row;
            row.v = v;
#pragma unroll
            for (int i = 0; i < GNS_KWMAX; i++) row.k[i] = __builtin_bswap32(r[1 + i] & tail_mask(D.K, i));
            if constexpr (ExSelOf<SL...>::kSigned)  // the sign rides in key byte 39, which no key has (K <= 37):
                row.k[GNS_KWMAX - 1] |= (long long)(metric ? f.bytes[s] : f.pkts[s]) < 0 ? 1u : 0u;  // below every key bit
            rows[q] = row;
        }
    }
}
__global__ __launch_bounds__(256) void k_exq_hh_out(const ExHhRow *rows, uint64_t n, uint32_t K, uint8_t *keys,
                                                    unsigned long long *vals) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const ExHhRow row = rows[p];
    for (uint32_t j = 0; j < K; j++) {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < GNS_KWMAX; i++) w = (j >> 2) == (uint32_t)i ? row.k[i] : w;
        keys[p * K + j] = (uint8_t)(w >> (8u * (3u - (j & 3u))));
    }
    vals[p] = row.v;
}

// gns_ex_movers after HH4: the magnitudes become the signed changes (ExSelSigned's sign bit)
__global__ __launch_bounds__(256) void k_exq_mv_sign(const ExHhRow *rows, uint64_t n, unsigned long long *vals) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    if (rows[p].k[GNS_KWMAX - 1] & 1u) vals[p] = 0ull - vals[p];
}

// table growth: per-flow state follows its record to the new slot (gns_dict.hip remap)
__global__ __launch_bounds__(256) void k_ex_permute(FlowState o, uint64_t slots, const uint32_t *remap, FlowState f) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const uint32_t t = remap[s];
    if (t >= kDictMarked) return;  // dropped (GNS_ID_NONE) or never reinserted
    f.pkts[t] = o.pkts[s]; f.bytes[t] = o.bytes[s]; f.first[t] = o.first[s]; f.last[t] = o.last[s];
    f.start[t] = o.start[s]; f.end[t] = o.end[s];
}

__global__ __launch_bounds__(256) void k_ex_init(FlowState f, uint64_t slots) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    f.pkts[s] = 0; f.bytes[s] = 0; f.first[s] = ~0ull; f.last[s] = 0; f.start[s] = 0; f.end[s] = 0;
}

// ---------------------------------------------------------------------------
// History (gns_ex_hist_*): an append-only log of snapshot rows.  A log row is a view's row
// -- record at stride RW, start, end, pkts, bytes -- with two version words: the snapshot
// that wrote it and the snapshot that next wrote the same key (kHistOpen: none yet).  The key
// index is a dictionary of the history's own (HistIndex, gns_histindex.hpp) with one head word
// per slot, the newest log row of that key.  "The latest row of each flow as of snapshot s" is then
// written <= s < superseded, tested in the scans of the query plane (ExSelAsOf).
//   A1 HistIndex::resolve the view's key words -> index slots (growth and retry as gns_ex_merge)
//   A2 k_exh_link         view row i -> log row base + i, stamped written = S; the row is
//                         swapped into its key's head word and the row it displaced is
//                         stamped superseded = S.  Keys are distinct within a view, so no two
//                         lanes touch one head word.
// Nothing the link writes is visible to a query before the host publishes S: rows at and
// beyond the published count are outside every scan, and a displaced row stays live for every
// s < S.
// ---------------------------------------------------------------------------
struct ExHistLog {
    DictDev L;    // rec / RW / K: the records
    FlowState f;  // pkts, bytes, start, end (first / last stay NULL)
    uint32_t *written, *superseded;
    uint64_t cap;
};
__global__ __launch_bounds__(256) void k_exh_link(DictDev V, FlowState vf, uint64_t n, const uint32_t *ids,
                                                  uint32_t *head, uint32_t slots, ExHistLog G, uint64_t base, uint32_t S,
                                                  uint32_t *fresh) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t r = base + i;
    uint32_t id = GNS_ID_NONE;
    bool isnew = false;
    if (i < n && r < G.cap) {
        const uint4 *q = reinterpret_cast<const uint4 *>(V.rec + i * V.RW);
        uint4 *o = reinterpret_cast<uint4 *>(G.L.rec + r * V.RW);
#pragma unroll
        for (int w = 0; w < 4; w++)
            if (4u * w < V.RW) o[w] = q[w];
        G.f.pkts[r] = vf.pkts[i]; G.f.bytes[r] = vf.bytes[i]; G.f.start[r] = vf.start[i]; G.f.end[r] = vf.end[i];
        G.written[r] = S;
        G.superseded[r] = kHistOpen;
        id = ids[i];
        if (id < slots) {  // (always: every id of the append was resolved before the link)
            const uint32_t old = head[id];
            head[id] = (uint32_t)r;
            if (old == kHistOpen) isnew = true;
            else if (old < base) G.superseded[old] = S;
        }
    }
    const uint64_t m = __ballot(isnew);  // keys new to the history: one add per wave
    if (m && __lane_id() == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(fresh, (uint32_t)__popcll(m));
}
// gns_ex_hist_append_rows: host rows instead of a view's.  The state words already lie in the
// log at base + i (copied there behind the published rows); the record is the one the resolve
// found or claimed in the index.  Two rows of one call with one key would share a head word,
// which the link must not meet: HistIndex::check_unique refuses the call first.
__global__ __launch_bounds__(256) void k_exh_link_rows(DictDev I, uint64_t n, const uint32_t *ids, uint32_t *head,
                                                       uint32_t slots, ExHistLog G, uint64_t base, uint32_t S,
                                                       uint32_t *fresh) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t r = base + i;
    bool isnew = false;
    if (i < n && r < G.cap) {
        const uint32_t id = ids[i];
        if (id < slots) {  // (always: every id of the append was resolved before the link)
            const uint4 *q = reinterpret_cast<const uint4 *>(I.rec + (uint64_t)id * I.RW);
            uint4 *o = reinterpret_cast<uint4 *>(G.L.rec + r * I.RW);
#pragma unroll
            for (int w = 0; w < 4; w++)
                if (4u * w < I.RW) o[w] = w < 3 ? q[w] : make_uint4(0, 0, 0, 0);
            G.written[r] = S;
            G.superseded[r] = kHistOpen;
            const uint32_t old = head[id];
            head[id] = (uint32_t)r;
            if (old == kHistOpen) isnew = true;
            else if (old < base) G.superseded[old] = S;
        }
    }
    const uint64_t m = __ballot(isnew);
    if (m && __lane_id() == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(fresh, (uint32_t)__popcll(m));
}

// gns_ex_hist_trim.  The kept rows of the old log O -- of the expired prefix [0, R) those still
// live as of snapshot s_last (fold; their ranks come from k_exhv_count over the prefix and the
// scan, as V1 / V2), and every row from R on -- move stably into the new log G: a prefix row to
// its rank, a suffix row to r - R + nbase.  Version words lose d; a word below d belongs to the
// base and becomes 0.  row0: the first row of the grid (0 whenever prefix rows are ranked: block
// b is then the count's block b).  newrow[r] = where prefix row r went (kHistOpen: dropped), for
// the head words.  O is only read: a failed trim leaves it as it was.
struct ExHistTrim {
    uint64_t rows, R, nbase, row0;
    uint32_t s_last, d, nb;
    int fold;
};
__global__ __launch_bounds__(256) void k_exh_trim_move(ExHistLog O, ExHistTrim t, const uint32_t *off, ExHistLog G,
                                                       uint32_t *newrow) {
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t r = t.row0 + (uint64_t)blockIdx.x * 256 + tid;
    const bool prefix = r < t.R;
    const bool sel = prefix && t.fold && O.superseded[r] > t.s_last;
    const uint64_t m = __ballot(sel);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (r >= t.rows) return;
    uint64_t nr = r - t.R + t.nbase;
    if (prefix) {
        nr = kHistOpen;
        if (sel) {
            nr = off[exv_cell(blockIdx.x, t.nb)] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            for (uint32_t w = 0; w < wave; w++) nr += s_w[w];
        }
        if (newrow) newrow[r] = (uint32_t)nr;
        if (!sel) return;
    }
    if (nr >= G.cap) return;
    const uint32_t RW = O.L.RW;
    const uint4 *q = reinterpret_cast<const uint4 *>(O.L.rec + r * RW);
    uint4 *o = reinterpret_cast<uint4 *>(G.L.rec + nr * RW);
#pragma unroll
    for (int w = 0; w < 4; w++)
        if (4u * w < RW) o[w] = q[w];
    G.f.pkts[nr] = O.f.pkts[r]; G.f.bytes[nr] = O.f.bytes[r]; G.f.start[nr] = O.f.start[r]; G.f.end[nr] = O.f.end[r];
    const uint32_t a = O.written[r], b = O.superseded[r];
    G.written[nr] = max(a, t.d) - t.d;
    G.superseded[nr] = b == kHistOpen ? kHistOpen : b - t.d;
}
// where the row a head word names went
__device__ __forceinline__ uint32_t exh_trim_head(uint32_t h, const ExHistTrim &t, const uint32_t *newrow) {
    if (h == kHistOpen) return kHistOpen;
    if (h >= t.R) return (uint32_t)(h - t.R + t.nbase);
    return newrow ? newrow[h] : kHistOpen;
}
// the slots whose key keeps a row name themselves (dict_rebuild's mark list); the others are counted
__global__ __launch_bounds__(256) void k_exh_trim_marks(const uint32_t *head, uint64_t slots, ExHistTrim t,
                                                        const uint32_t *newrow, uint32_t *ids, uint32_t *forgot) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool gone = false;
    if (s < slots) {
        const uint32_t h = head[s], n = exh_trim_head(h, t, newrow);
        ids[s] = n != kHistOpen ? (uint32_t)s : GNS_ID_NONE;
        gone = h != kHistOpen && n == kHistOpen;
    }
    const uint64_t m = __ballot(gone);
    if (m && __lane_id() == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(forgot, (uint32_t)__popcll(m));
}
// the new head words: at the slot the rebuild gave the key (remap == nullptr: the slot it has)
__global__ __launch_bounds__(256) void k_exh_trim_heads(const uint32_t *head, uint64_t slots, ExHistTrim t,
                                                        const uint32_t *newrow, const uint32_t *remap, uint32_t *nh) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const uint32_t n = exh_trim_head(head[s], t, newrow);
    if (!remap) { nh[s] = n; return; }
    const uint32_t to = remap[s];
    if (to >= kDictMarked) return;
    nh[to] = n;
}

// gns_ex_merge: row i is one pseudo-record at stream position base + i.  Counts add
// (u64 wrap); first / last keep the stream-order rule among the rows of one call and
// against the table (an existing flow's first lies below base), and the rows that
// hold a flow's first / last position give it their timestamps.
__global__ __launch_bounds__(256) void k_ex_merge_add(const uint32_t *ids, uint64_t n, const unsigned long long *pkts,
                                                      const unsigned long long *bytes, unsigned long long base,
                                                      FlowState f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    if (id == GNS_ID_NONE) return;  // a row without packets
    atomicAdd(&f.pkts[id], pkts[i]);
    atomicAdd(&f.bytes[id], bytes[i]);
    atomicMin(&f.first[id], base + i);
    atomicMax(&f.last[id], base + i + 1);
}

__global__ __launch_bounds__(256) void k_ex_merge_times(const uint32_t *ids, uint64_t n, const long long *start,
                                                        const long long *end, unsigned long long base, FlowState f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    if (id == GNS_ID_NONE) return;
    if (f.first[id] == base + i) f.start[id] = start[i];
    if (f.last[id] == base + i + 1) f.end[id] = end[i];
}

// ---------------------------------------------------------------------------
// Roll-up (gns_ex_rollup): the flows of a source table projected onto the key
// layout of another handle and merged there group by group.  The reference
// answers a coarser question with one task per key layout, every task fed every
// packet (manager.go:232-244), or with GROUP BY over stored rows
// (querier.go:251-319); here the coarser table is derived from the resident one.
// Per piece of source slots:
//   R1 k_exr_project  occupied slot -> dense row {projected key, pkts, bytes,
//                     first, last, start, end} (wave ballot, one atomic per wave)
//   R2 dict_resolve_keys on the destination (merge's growth-and-retry loop)
//   R3 k_exr_add      counts add, first / last = min / max of the positions
//                     mapped behind the destination's stream end
//   R4 k_exr_times    the row that holds a group's first / last position gives
//                     it its start / end
// first / last are monotone under R3 across pieces, so a later piece with a
// smaller first overwrites start and one with a larger first writes nothing;
// positions are unique per record across flows, so no two rows of a group tie.
// ---------------------------------------------------------------------------
// The plan as R1 takes it.  Plain: the gather alone, read as kernel-argument scalars.
// PX (gns_ex_rollup_prefix: the projected key's IP fields masked to a prefix): the whole
// RollRow, which the kernel keeps in LDS (one broadcast read per table byte) -- its 160 bytes
// as kernel-argument scalars would be live across the unrolled gather, where the 74 bytes of
// k_spr_project's spilled 270 SGPRs.
template <bool PX>
struct ExrPlan {
    uint32_t K, KW;  // destination key bytes / words (a row's key takes KW words)
    uint8_t t[40];   // proj_word<false>'s table: source key byte of destination key byte j
};
template <>
struct ExrPlan<true> {
    uint32_t K, KW;
    uint8_t ipoff[4];  // byte offset of SrcIP / DstIP in the source key; 0xFF: not read
    union {            // proj_word<true>'s tables; as words for the copy into LDS
        uint8_t t[sizeof(RollRow)];
        uint32_t w[sizeof(RollRow) / 4];
    };
};
struct ExrRows {
    uint32_t *keys, *ids, *cnt;
    unsigned long long *pkts, *bytes, *first, *last;
    long long *start, *end;
};

// grid covers slots [s0, s1); at most s1 - s0 rows are appended (R.cnt zeroed by the host).
// PX: a lane takes one IPv4 flag per IP field of its source key -- spr_encode_ip's test, on the
// unmasked bytes -- and proj_word<true> masks by it: IP fields at any offset.
template <bool PX>
__global__ __launch_bounds__(256) void k_exr_project(DictDev S, FlowState sf, uint64_t s0, uint64_t s1, ExrPlan<PX> pl,
                                                     ExrRows R) {
    __shared__ uint32_t s_k[GNS_KWMAX][256];  // proj_fill_column
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint8_t *t;
    if constexpr (PX) {
        __shared__ uint32_t s_pw[40];  // g, fld, m4, m6
        if (tid < 40) s_pw[tid] = pl.w[tid];
        __syncthreads();  // before any wave leaves
        t = reinterpret_cast<const uint8_t *>(s_pw);
    } else {
        t = pl.t;  // uniform: scalar loads of the kernel argument
    }
    const uint64_t s = s0 + (uint64_t)blockIdx.x * 256 + tid;
    unsigned long long pk = 0;
    uint32_t r[12];
    bool occ = false;
    if (s < s1) {
        load_record(S, (uint32_t)s, r);
        pk = sf.pkts[s];
        occ = r[0] != 0u && pk != 0ull;  // k_ex_list's occupancy rule
    }
    const uint64_t m = __ballot(occ);
    if (m == 0) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(R.cnt, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (!occ) return;
    const uint64_t row = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    proj_fill_column(s_k, tid, r);
    uint32_t v4 = 0;  // bit f: IP field f of this flow is IPv4
    if constexpr (PX) {
#pragma unroll
        for (int f = 0; f < 2; f++)  // SrcIP, DstIP: a key of <= 37 bytes holds two IP fields at most
            if (pl.ipoff[f] != 0xFFu) v4 |= (px_is_v4(s_k, tid, pl.ipoff[f]) ? 1u : 0u) << f;
    }
#pragma unroll
    for (int i = 0; i < GNS_KWMAX; i++) {
        if ((uint32_t)i >= pl.KW) break;  // uniform
        R.keys[row * pl.KW + i] = proj_word<PX>(s_k, tid, t, v4, pl.K, i);
    }
    R.pkts[row] = pk; R.bytes[row] = sf.bytes[s]; R.first[row] = sf.first[s]; R.last[row] = sf.last[s];
    R.start[row] = sf.start[s]; R.end[row] = sf.end[s];
}

// R3.  A roll-up to a few groups would send every row's four atomics to a few addresses.
// Rows of one id are combined before anything leaves the CU (as k_exq_aggregate): the ids
// most lanes of a wave share are reduced across the wave, every id goes through a small LDS
// table of the workgroup's partials, and the table leaves as one set of global atomics per id
// and workgroup.  An id that finds no room in the table goes to global memory directly (many
// groups: those atomics do not collide).  Integer add / min / max: bit-exact in any order.
constexpr uint32_t kExrTabBits = 9, kExrTab = 1u << kExrTabBits;
constexpr int kExrPeel = 6;  // wave reductions per row of 64: the ids of at least 4 lanes

struct ExrLds {
    uint32_t id[kExrTab];
    unsigned long long pk[kExrTab], by[kExrTab], fi[kExrTab], la[kExrTab];
};

__device__ __forceinline__ void exr_merge(ExrLds &t, const FlowState &f, uint32_t id, unsigned long long pk,
                                          unsigned long long by, unsigned long long fi, unsigned long long la) {
    uint32_t h = (id * 0x9E3779B1u) >> (32 - kExrTabBits);
    for (int p = 0; p < 4; p++) {
        const uint32_t old = atomicCAS(&t.id[h], GNS_ID_NONE, id);
        if (old == GNS_ID_NONE || old == id) {
            atomicAdd(&t.pk[h], pk);
            atomicAdd(&t.by[h], by);
            atomicMin(&t.fi[h], fi);
            atomicMax(&t.la[h], la);
            return;
        }
        h = (h + 1u) & (kExrTab - 1u);
    }
    atomicAdd(&f.pkts[id], pk);
    atomicAdd(&f.bytes[id], by);
    atomicMin(&f.first[id], fi);
    atomicMax(&f.last[id], la);
}

__global__ __launch_bounds__(256) void k_exr_add(ExrRows R, uint64_t n, unsigned long long B, FlowState f) {
    __shared__ ExrLds t;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < kExrTab; i += 256) { t.id[i] = GNS_ID_NONE; t.pk[i] = 0; t.by[i] = 0; t.fi[i] = ~0ull; t.la[i] = 0; }
    __syncthreads();
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < n; i0 += (uint64_t)gridDim.x * 256) {  // block-uniform
        const uint64_t i = i0 + tid;
        uint32_t id = GNS_ID_NONE;
        unsigned long long pk = 0, by = 0, fi = ~0ull, la = 0;
        if (i < n) id = R.ids[i];
        bool pending = id != GNS_ID_NONE;
        if (pending) { pk = R.pkts[i]; by = R.bytes[i]; fi = B + R.first[i]; la = B + R.last[i]; }
        uint64_t todo = __ballot(pending);
        for (int round = 0; round < kExrPeel && todo; round++) {  // wave-uniform
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const uint32_t lid = (uint32_t)__shfl((int)id, lead);
            const bool in = pending && id == lid;
            const uint64_t same = __ballot(in);
            todo &= ~same;
            if (__popcll(same) < 4) continue;  // these lanes merge their own rows below
            const unsigned long long tp = __ockl_wfred_add_u64(in ? pk : 0ull);
            const unsigned long long tb = __ockl_wfred_add_u64(in ? by : 0ull);
            const unsigned long long tf = __ockl_wfred_min_u64(in ? fi : ~0ull);
            const unsigned long long tl = __ockl_wfred_max_u64(in ? la : 0ull);
            if ((int)lane == lead) exr_merge(t, f, lid, tp, tb, tf, tl);
            pending = pending && !in;
        }
        if (pending) exr_merge(t, f, id, pk, by, fi, la);
    }
    __syncthreads();
    for (uint32_t h = tid; h < kExrTab; h += 256) {
        const uint32_t id = t.id[h];
        if (id == GNS_ID_NONE) continue;
        atomicAdd(&f.pkts[id], t.pk[h]);
        atomicAdd(&f.bytes[id], t.by[h]);
        atomicMin(&f.first[id], t.fi[h]);
        atomicMax(&f.last[id], t.la[h]);
    }
}

__global__ __launch_bounds__(256) void k_exr_times(ExrRows R, uint64_t n, unsigned long long B, FlowState f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = R.ids[i];
    if (id == GNS_ID_NONE) return;
    if (f.first[id] == B + R.first[i]) f.start[id] = R.start[i];
    if (f.last[id] == B + R.last[i]) f.end[id] = R.end[i];
}

// ---------------------------------------------------------------------------
// History roll-up (gns_ex_hist_rollup): the rows of a history's log LIVE as of snapshot
// s -- the rows gns_ex_hist_snapshot lists, the reference's argMax(..., Timestamp) with
// Timestamp <= T -- projected onto another handle's key layout and merged there as the
// reference's GROUP BY over stored rows has it (querier.go:251-372): counts add, StartTime
// is the group's minimum and EndTime its maximum.  Log rows carry no stream positions, so
// the stream-order rule of gns_ex_rollup has nothing to order by; min / max does not depend
// on the order of rows inside a snapshot.  Log row r stands at stream position B + r.
// Per piece of log rows:
//   H1 k_exh_project  live row -> dense row {projected key, pkts, bytes, r, start, end}
//                     (R1 with ExSelAsOf as the selection and the log as the source)
//   R2 ex_resolve_rows on the destination
//   H2 k_exh_seed     a slot no row has reached yet (first == ~0: k_ex_init's, or a
//                     growth's) gets start = int64 max, end = int64 min, so that the zeros
//                     it was created with take no part in the min / max
//   H3 k_exh_add      counts add, first / last = min / max of the positions, start / end
//                     = signed min / max: R3 with two more columns, and no R4
// H2 reads first and writes start / end, H3 is the first to write first: every row of a new
// slot sees it as new and stores the same two seeds, whichever lanes get there.
// ---------------------------------------------------------------------------
// The selection of a window (T0, T1] (gns_ex_hist_rollup_between), HistPlan::between's: lo =
// s0 + 1.  A row (written a, superseded b) is a PLUS row when s0 < a <= s1 < b and a MINUS row
// when a <= s0 < b <= s1.  The log is in snapshot order, so a row below minus_end has a <= s0
// and a row from there to the scan's end s0 < a <= s1: one version word per row decides, and a
// row live at both times (the common one) is never loaded.
struct ExSelBetween {
    const uint32_t *superseded;
    uint32_t lo, s1;
    uint64_t minus_end;
    __device__ __forceinline__ void pick(uint64_t row, bool &take, bool &minus) const {
        const uint32_t b = superseded[row];
        minus = row < minus_end;
        take = minus ? (lo <= b && b <= s1) : s1 < b;
    }
};

// H1.  SEL = ExSelAsOf (the live rows) or ExSelBetween (plus and minus rows, r1 <= the rows as of
// sel.s1; a minus row enters as {-pkts, -bytes, start = int64 max, end = int64 min}: it subtracts
// under H3's wrapping adds and takes no part in its min / max, so H2 and H3 run unchanged).
// grid covers log rows [r0, r1), r1 <= the rows as of sel.s; at most r1 - r0 rows are appended
// (R.cnt zeroed by the host).  A wave none of whose rows is selected loads no record.
// R.first[row] = the log row; R.last is not written.
template <bool PX, class SEL = ExSelAsOf>
__global__ __launch_bounds__(256) void k_exh_project(DictDev L, FlowState lf, SEL sel, uint64_t r0, uint64_t r1,
                                                     ExrPlan<PX> pl, ExrRows R) {
    constexpr bool kBetween = std::is_same<SEL, ExSelBetween>::value;
    __shared__ uint32_t s_k[GNS_KWMAX][256];  // proj_fill_column
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint8_t *t;
    if constexpr (PX) {
        __shared__ uint32_t s_pw[40];  // g, fld, m4, m6 (not kernel-argument scalars: see ExrPlan)
        if (tid < 40) s_pw[tid] = pl.w[tid];
        __syncthreads();  // before any wave leaves
        t = reinterpret_cast<const uint8_t *>(s_pw);
    } else {
        t = pl.t;
    }
    const uint64_t r = r0 + (uint64_t)blockIdx.x * 256 + tid;
    bool live = false;
    [[maybe_unused]] bool minus = false;
    if constexpr (kBetween) {
        if (r < r1) sel.pick(r, live, minus);
    } else {
        bool seen = false;
        if (r < r1) sel.test(r, seen, live);
    }
    const uint64_t m = __ballot(live);
    if (m == 0) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(R.cnt, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (!live) return;
    const uint64_t row = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    uint32_t w[12];
    load_record(L, (uint32_t)r, w);
    proj_fill_column(s_k, tid, w);
    uint32_t v4 = 0;  // bit f: IP field f of this flow is IPv4
    if constexpr (PX) {
#pragma unroll
        for (int f = 0; f < 2; f++)
            if (pl.ipoff[f] != 0xFFu) v4 |= (px_is_v4(s_k, tid, pl.ipoff[f]) ? 1u : 0u) << f;
    }
#pragma unroll
    for (int i = 0; i < GNS_KWMAX; i++) {
        if ((uint32_t)i >= pl.KW) break;  // uniform
        R.keys[row * pl.KW + i] = proj_word<PX>(s_k, tid, t, v4, pl.K, i);
    }
    if constexpr (kBetween) {
        const unsigned long long pk = lf.pkts[r], by = lf.bytes[r];
        R.pkts[row] = minus ? 0ull - pk : pk; R.bytes[row] = minus ? 0ull - by : by; R.first[row] = r;
        R.start[row] = minus ? INT64_MAX : lf.start[r]; R.end[row] = minus ? INT64_MIN : lf.end[r];
    } else {
        R.pkts[row] = lf.pkts[r]; R.bytes[row] = lf.bytes[r]; R.first[row] = r;
        R.start[row] = lf.start[r]; R.end[row] = lf.end[r];
    }
}

__global__ __launch_bounds__(256) void k_exh_seed(const uint32_t *ids, uint64_t n, FlowState f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    if (id == GNS_ID_NONE) return;
    if (f.first[id] == ~0ull) { f.start[id] = INT64_MAX; f.end[id] = INT64_MIN; }
}

// H3's workgroup table: R3's, and the two time columns as unsigned words with the sign bit
// flipped (kQSign, as the query plane reduces them), which keeps the signed order under the
// unsigned wave reductions and LDS atomics.  They leave the CU as signed 64-bit atomics on the
// raw words of the table.  ~26 KB.
struct ExhLds {
    uint32_t id[kExrTab];
    unsigned long long pk[kExrTab], by[kExrTab], fi[kExrTab], la[kExrTab], st[kExrTab], en[kExrTab];
};

struct ExhRow {
    unsigned long long pk, by, fi, la, st, en;  // st / en: sign-flipped
};

__device__ __forceinline__ void exh_global(const FlowState &f, uint32_t id, const ExhRow &v) {
    atomicAdd(&f.pkts[id], v.pk);
    atomicAdd(&f.bytes[id], v.by);
    atomicMin(&f.first[id], v.fi);
    atomicMax(&f.last[id], v.la);
    atomicMin(&f.start[id], (long long)(v.st ^ kQSign));
    atomicMax(&f.end[id], (long long)(v.en ^ kQSign));
}

__device__ __forceinline__ void exh_merge(ExhLds &t, const FlowState &f, uint32_t id, const ExhRow &v) {
    uint32_t h = (id * 0x9E3779B1u) >> (32 - kExrTabBits);
    for (int p = 0; p < 4; p++) {
        const uint32_t old = atomicCAS(&t.id[h], GNS_ID_NONE, id);
        if (old == GNS_ID_NONE || old == id) {
            atomicAdd(&t.pk[h], v.pk);
            atomicAdd(&t.by[h], v.by);
            atomicMin(&t.fi[h], v.fi);
            atomicMax(&t.la[h], v.la);
            atomicMin(&t.st[h], v.st);
            atomicMax(&t.en[h], v.en);
            return;
        }
        h = (h + 1u) & (kExrTab - 1u);
    }
    exh_global(f, id, v);
}

// row i stands at stream position B + R.first[i]; the stored `last` word is one past it, as
// everywhere (k_ex_merge_add)
__global__ __launch_bounds__(256) void k_exh_add(ExrRows R, uint64_t n, unsigned long long B, FlowState f) {
    __shared__ ExhLds t;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < kExrTab; i += 256) {
        t.id[i] = GNS_ID_NONE; t.pk[i] = 0; t.by[i] = 0; t.fi[i] = ~0ull; t.la[i] = 0; t.st[i] = ~0ull; t.en[i] = 0;
    }
    __syncthreads();
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < n; i0 += (uint64_t)gridDim.x * 256) {  // block-uniform
        const uint64_t i = i0 + tid;
        uint32_t id = GNS_ID_NONE;
        ExhRow v{0, 0, ~0ull, 0, ~0ull, 0};
        if (i < n) id = R.ids[i];
        bool pending = id != GNS_ID_NONE;
        if (pending) {
            v.pk = R.pkts[i]; v.by = R.bytes[i]; v.fi = B + R.first[i]; v.la = v.fi + 1;
            v.st = (unsigned long long)R.start[i] ^ kQSign; v.en = (unsigned long long)R.end[i] ^ kQSign;
        }
        uint64_t todo = __ballot(pending);
        for (int round = 0; round < kExrPeel && todo; round++) {  // wave-uniform
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const uint32_t lid = (uint32_t)__shfl((int)id, lead);
            const bool in = pending && id == lid;
            const uint64_t same = __ballot(in);
            todo &= ~same;
            if (__popcll(same) < 4) continue;  // these lanes merge their own rows below
            ExhRow w;
            w.pk = __ockl_wfred_add_u64(in ? v.pk : 0ull);
            w.by = __ockl_wfred_add_u64(in ? v.by : 0ull);
            w.fi = __ockl_wfred_min_u64(in ? v.fi : ~0ull);
            w.la = __ockl_wfred_max_u64(in ? v.la : 0ull);
            w.st = __ockl_wfred_min_u64(in ? v.st : ~0ull);
            w.en = __ockl_wfred_max_u64(in ? v.en : 0ull);
            if ((int)lane == lead) exh_merge(t, f, lid, w);
            pending = pending && !in;
        }
        if (pending) exh_merge(t, f, id, v);
    }
    __syncthreads();
    for (uint32_t h = tid; h < kExrTab; h += 256) {
        const uint32_t id = t.id[h];
        if (id == GNS_ID_NONE) continue;
        exh_global(f, id, ExhRow{t.pk[h], t.by[h], t.fi[h], t.la[h], t.st[h], t.en[h]});
    }
}

}  // namespace gns

using namespace gns;

// Scratch of the read side (gns_ex_aggregate, gns_ex_heavy_hitters, a view's snapshot).
// The handle's own calls take one per call, sized exactly, copy straight to the caller's
// memory and free it on return, as they always have.  A snapshot view keeps one (keep):
// its buffers only grow, to twice the request, and every host copy goes through pinned
// staging -- hipFree synchronizes the device and a copy to pageable memory blocks in the
// runtime, and neither may happen under a reader while the handle ingests.
struct ExRead {
    bool keep = false;
    ExQFilter *df = nullptr;
    unsigned long long *da = nullptr, *dv = nullptr;
    uint32_t *dh = nullptr;
    ExHhRow *rows[2] = {nullptr, nullptr};
    uint8_t *tmp = nullptr, *dk = nullptr;
    uint64_t df_n = 0, da_n = 0, dv_n = 0, dh_n = 0, rows_n[2] = {0, 0}, tmp_n = 0, dk_n = 0;
    PinnedOut po;  // keep: pinned host staging

    template <class T>
    int buf(T **p, uint64_t &have, uint64_t need) {
        if (need <= have && *p) return GNS_OK;
        dfree(*p);
        *p = nullptr;
        have = 0;
        const uint64_t n = std::max<uint64_t>(keep ? 2 * need : need, 1);
        GNS_TRY(dalloc_t(p, n));
        have = n;
        return GNS_OK;
    }
    int init_keep() {
        keep = true;
        return po.reserve(2 * kPinChunk);
    }
    void free_all() {
        dfree(df); dfree(da); dfree(dv); dfree(dh); dfree(rows[0]); dfree(rows[1]); dfree(tmp); dfree(dk);
        df = nullptr; da = dv = nullptr; dh = nullptr; rows[0] = rows[1] = nullptr; tmp = dk = nullptr;
        df_n = da_n = dv_n = dh_n = rows_n[0] = rows_n[1] = tmp_n = dk_n = 0;
        po.free_all();
    }
    // Device bytes -> the caller's host memory.  !keep: straight out (the caller synchronizes
    // the stream).  keep: through the pinned buffer; complete on return.
    int copy_out(void *dst, const void *src, size_t bytes, hipStream_t s) {
        if (keep) return po.copy_out(dst, src, bytes, s);
        GNS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        return GNS_OK;
    }
};

struct gns_ex {
    int device = 0;
    bool force_list = false;  // GNS_EX_LIST=1: T/D over the touched list at any table size (tests)
    hipStream_t stream = nullptr;
    KeyPlanN kp{};
    uint32_t K = 0;
    DictDev D{};
    uint64_t slots = 0;
    uint64_t claimed = 0;                    // D.ctl[0] as of the last batch
    uint32_t *dctl = nullptr;
    DictScratch dsc;
    unsigned long long *stats_bak = nullptr;
    uint64_t n_grow = 0, n_retry = 0;
    double grow_ms = 0.0;
    FlowState f{};
    uint32_t epoch = 0;
    uint64_t pkt = 0, batches = 0;
    uint64_t merged = 0;                     // rows gns_ex_merge placed in the stream: positions are pkt + merged
    uint64_t bmax = 0;
    uint32_t nblk_max = 0;
    uint64_t *sk[2] = {nullptr, nullptr};    // X1 block regions of tail words; the same partitioned by bin
    uint32_t *hot_ids = nullptr;             // [kExHot] designated flows (GNS_ID_NONE: unused slot)
    unsigned long long *hot_tab = nullptr;   // [kExHotTab] their lookup table
    ExHotPart *hpart = nullptr;              // [kExHot][nblk_max]
    uint32_t *hctl = nullptr;                // [0..511] count histogram, [512] threshold, [513] count, [514] tail words, [515] touched
    uint32_t *touch = nullptr;               // [bmax + kExHot] flows the batch touched (T, D)
    uint32_t *ccnt = nullptr;                // [nblk_max] X1 region word counts
    bool warm = false;                       // flows designated (a batch ran since create / reset / growth)
    uint32_t *ph = nullptr, *pgs = nullptr, *pb = nullptr;  // P histograms / offsets, group sums, bin starts
    uint32_t key_bits = 0;                   // flow field bits: flow ids < slots, invalid = slots
    uint32_t sb = 0, ib = 0;                 // sort word: wire length bits, packet index bits
    uint64_t *pend[2] = {nullptr, nullptr};
    uint32_t *pcnt[2] = {nullptr, nullptr};
    uint32_t *ptotal = nullptr;
    unsigned long long *stats = nullptr;
    uint32_t *h_pin = nullptr;
    HostStage stage;
    CompactInput compact;  // compact records: the staged side array, the 16-byte form's sizes
    QueryStage qs;         // host queries' keys and answers on the device
    StageTimer timer;
};

// the table as another engine's kernels may read it (gns_exsrc.hpp)
void gns::ex_table_ref(const gns_ex *ex, ExTableRef *out) {
    out->device = ex->device;
    out->stream = ex->stream;
    out->kp = ex->kp;
    out->D = ex->D;
    out->slots = ex->slots;
    out->pkts = ex->f.pkts;
    out->first = ex->f.first;
    out->pos = ex->pkt + ex->merged;  // the next stream position (ex_run_batch, gns_ex_merge)
}

// A dense copy of the flows one refresh selected: records at stride RW and the four
// exported state arrays, `cap` rows of room, the row count on the device (*total) until a
// reader fetches it.  Nothing in it points into the handle's table.
struct gns_ex_view : ViewCore {
    gns_ex *ex = nullptr;
    bool fresh = false;    // refreshed at least once
    bool counted = false;  // n holds this refresh's row count
    uint64_t n = 0;
    DictDev D{};
    FlowState f{};         // (first / last stay NULL: no query reads them)
    uint64_t cap = 0;
    uint32_t *scan = nullptr;  // V1's block counts / offsets, then the scan's group sums and bin totals
    uint64_t scan_n = 0;
    uint32_t *total = nullptr;
    ExRead rd;
};

// The history of one key layout: the log, the key index and its head words, and the reader's
// scratch.  Its stream, mutex and pinned staging are its own, as a view's: appends and queries
// from any thread are serialised by the mutex and allocate nothing once warm.
struct gns_ex_hist : ViewCore {
    int device = 0;
    KeyPlanN kp{};
    uint32_t K = 0;
    HistPlan plan;             // timestamps, published rows (host)
    ExHistLog log{};           // cap rows of room
    HistIndex ix;              // the key index
    uint64_t keys = 0;
    uint32_t *head = nullptr;  // [ix.slots] newest log row of the slot's key (kHistOpen: none)
    uint64_t n_log_grow = 0, rows_trimmed = 0;
    // as-of snapshot: V1's counts and the scan's sums, the total, the compacted rows
    uint32_t *scan = nullptr, *total = nullptr;
    uint64_t scan_n = 0;
    DictDev SD{};
    FlowState sf{};
    uint64_t scap = 0;
    ExRead rd;
};

namespace {

void ex_free_all(gns_ex *ex) {
    dfree(ex->D.rec); dfree(ex->f.pkts); dfree(ex->f.bytes); dfree(ex->f.first); dfree(ex->f.last);
    dfree(ex->f.start); dfree(ex->f.end); dfree(ex->pend[0]); dfree(ex->pend[1]);
    dfree(ex->pcnt[0]); dfree(ex->pcnt[1]); dfree(ex->ptotal); dfree(ex->stats); ex->stage.free_all();
    ex->compact.free_all();
    ex->qs.free_all();
    dfree(ex->sk[0]); dfree(ex->sk[1]); dfree(ex->ph); dfree(ex->pgs); dfree(ex->pb);
    dfree(ex->hot_ids); dfree(ex->touch); dfree(ex->hot_tab); dfree(ex->hpart); dfree(ex->hctl); dfree(ex->ccnt);
    dfree(ex->dctl); dfree(ex->stats_bak); ex->dsc.free_all();
    if (ex->h_pin) (void)hipHostFree(ex->h_pin);
    ex->timer.destroy();
    if (ex->stream) (void)hipStreamDestroy(ex->stream);
}

// no designated flows (after create / reset, and after a table growth renumbers the flows)
int ex_hot_clear(gns_ex *ex) {
    ex->warm = false;
    GNS_HIP(hipMemsetAsync(ex->hot_ids, 0xFF, kExHot * 4, ex->stream));
    GNS_HIP(hipMemsetAsync(ex->hot_tab, 0xFF, kExHotTab * 8, ex->stream));
    return GNS_OK;
}

int ex_clear(gns_ex *ex) {
    GNS_HIP(hipMemsetAsync(ex->D.rec, 0, ex->slots * ex->D.RW * 4, ex->stream));
    GNS_HIP(hipMemsetAsync(ex->dctl, 0, 16, ex->stream));
    ex->claimed = 0;
    GNS_HIP(hipMemsetAsync(ex->stats + 3, 0, sizeof(unsigned long long), ex->stream));  // dict-full word
    GNS_TRY(ex_hot_clear(ex));
    hipLaunchKernelGGL(k_ex_init, dim3((unsigned)((ex->slots + 255) / 256)), dim3(256), 0, ex->stream, ex->f,
                       ex->slots);
    GNS_HIP(hipGetLastError());
    return GNS_OK;
}

template <int KIND, int MODE>
int ex_run_batch(gns_ex *ex, const ExIn &xin, uint64_t n) {
    if (n == 0) return GNS_OK;
    hipStream_t s = ex->stream;
    const uint64_t pos = ex->pkt + ex->merged;  // stream position of the batch's first record
    const uint32_t nblk = (uint32_t)((n + kXChunk - 1) / kXChunk);
    ScopedStage total_stage(ex->timer, 5);
    GNS_HIP(hipMemsetAsync(ex->ptotal, 0, 8, s));
    GNS_HIP(hipMemsetAsync(ex->dctl + 1, 0, 4, s));  // abort flag of this batch
    if (++ex->epoch == 0) ex->epoch = 1;
    ExArgs x{};
    x.x = xin; x.n = n; x.kp = ex->kp; x.D = ex->D; x.epoch = ex->epoch;
    x.sk = ex->sk[0]; x.none_key = (uint32_t)ex->slots; x.hot_key = x.none_key + 1; x.sb = ex->sb; x.ib = ex->ib;
    x.hot_tab = ex->hot_tab; x.hpart = ex->hpart; x.ccnt = ex->ccnt; x.nblk = nblk;
    x.pend = ex->pend[0]; x.pend_cnt = ex->pcnt[0]; x.pend_total = ex->ptotal; x.stats = ex->stats;
    {
        ScopedStage st(ex->timer, 0);
        hipLaunchKernelGGL((k_ex_extract<KIND, MODE>), dim3(nblk), dim3(kXThreads), 0, s, x);
        GNS_HIP(hipGetLastError());
    }
    // resolve rounds; the first is queued behind X1 without a host round trip (X1
    // parks the flows displaced from their home slot; a block with none exits at once)
    int cur = 0;
    for (int round = 0;; round++) {
        if (round > 0) {
            GNS_HIP(hipMemcpyAsync(ex->h_pin, ex->ptotal + cur, 4, hipMemcpyDeviceToHost, s));
            GNS_HIP(hipMemcpyAsync(ex->h_pin + 2, ex->stats + 3, 8, hipMemcpyDeviceToHost, s));
            GNS_HIP(hipMemcpyAsync(ex->h_pin + 4, ex->dctl, 4, hipMemcpyDeviceToHost, s));
            GNS_HIP(hipStreamSynchronize(s));
            ex->claimed = ex->h_pin[4];
            if (ex->h_pin[2] | ex->h_pin[3]) { set_error("flow dictionary full; raise max_flows"); return GNS_E_FULL; }
            if (ex->h_pin[0] == 0) break;
        }
        if (round > 64) { set_error("dictionary resolve did not converge"); return GNS_E_FULL; }
        GNS_HIP(hipMemsetAsync(ex->ptotal + (cur ^ 1), 0, 4, s));
        if (++ex->epoch == 0) ex->epoch = 1;
        ExResolveArgs r{};
        r.x = x; r.x.epoch = ex->epoch;
        r.pend_in = ex->pend[cur]; r.cnt_in = ex->pcnt[cur];
        r.pend_out = ex->pend[cur ^ 1]; r.cnt_out = ex->pcnt[cur ^ 1]; r.total_out = ex->ptotal + (cur ^ 1);
        ScopedStage st(ex->timer, 1);
        hipLaunchKernelGGL((k_ex_resolve<KIND, MODE>), dim3(nblk), dim3(kXThreads), 0, s, r);
        GNS_HIP(hipGetLastError());
        cur ^= 1;
    }
    // T and D over the batch's touched-flow list once the table is large (a table that
    // grew with the period would make a full scan cost more than the batch); below
    // that, a sequential scan of every slot is cheaper than the list's random gathers
    uint32_t *touch = (ex->slots > kExListSlots || ex->force_list) ? ex->touch : nullptr;
    const uint32_t ks = ex->sb + ex->ib;
    // flow ids < slots = 2^(key_bits - 1): bin = id >> pshift
    const uint32_t pshift = ex->key_bits - 1 > kPBinBits ? ex->key_bits - 1 - kPBinBits : 0u;
    const uint32_t ng = (nblk + kPGroup - 1) / kPGroup;
    {
        ScopedStage st(ex->timer, 4);
        GNS_HIP(hipMemsetAsync(ex->hctl + 515, 0, 4, s));  // touched flows of this batch
        if (touch)
            hipLaunchKernelGGL(k_ex_hot_reduce<true>, dim3(kExHot), dim3(256), 0, s, ex->hpart, nblk, ex->hot_ids, pos,
                               ex->f, touch, ex->hctl + 515);
        else
            hipLaunchKernelGGL(k_ex_hot_reduce<false>, dim3(kExHot), dim3(256), 0, s, ex->hpart, nblk, ex->hot_ids, pos,
                               ex->f, touch, ex->hctl + 515);
        GNS_HIP(hipGetLastError());
    }
    {
        ScopedStage st(ex->timer, 2);
        const uint32_t none_key = (uint32_t)ex->slots;
        hipLaunchKernelGGL(k_ex_phist, dim3(nblk), dim3(256), 0, s, ex->sk[0], ex->ccnt, ks, pshift, none_key, ex->ph);
        hipLaunchKernelGGL(k_ex_pscan_a, dim3(ng), dim3(kPBins), 0, s, ex->ph, nblk, ex->pgs);
        hipLaunchKernelGGL(k_ex_pscan_b, dim3(1), dim3(kPBins), 0, s, ex->pgs, ng, ex->pb);
        hipLaunchKernelGGL(k_ex_pscan_c, dim3(ng), dim3(kPBins), 0, s, ex->ph, nblk, ex->pgs);
        hipLaunchKernelGGL(k_ex_pscatter, dim3(nblk), dim3(kPBins), 0, s, ex->sk[0], ex->ccnt, ex->ph, ks, pshift,
                           none_key, ex->sk[1]);
        GNS_HIP(hipGetLastError());
    }
    {
        ScopedStage st(ex->timer, 3);
        if (touch)
            hipLaunchKernelGGL(k_ex_pagg<true>, dim3(kPBins), dim3(kAggThreads), 0, s, ex->sk[1], ex->pb, ex->sb, ex->ib,
                           xin.in.sizes, pos, ex->f, touch, ex->hctl + 515);
        else
            hipLaunchKernelGGL(k_ex_pagg<false>, dim3(kPBins), dim3(kAggThreads), 0, s, ex->sk[1], ex->pb, ex->sb, ex->ib,
                           xin.in.sizes, pos, ex->f, touch, ex->hctl + 515);
        GNS_HIP(hipGetLastError());
    }
    {   // timestamps of the touched flows; the next batch's designated flows
        ScopedStage st(ex->timer, 4);
        if (touch) {
            const unsigned sg = (unsigned)std::min<uint64_t>((n + kExHot + 255) / 256, 4096);
            hipLaunchKernelGGL(k_ex_times_list, dim3(sg), dim3(256), 0, s, ex->f, touch, ex->hctl + 515, ex->slots, pos,
                               n, xin.ts);
            GNS_HIP(hipMemsetAsync(ex->hctl, 0, 514 * 4, s));
            GNS_HIP(hipMemsetAsync(ex->hot_ids, 0xFF, kExHot * 4, s));
            hipLaunchKernelGGL(k_exh_hist_list, dim3(std::min(sg, 2048u)), dim3(256), 0, s, ex->f.pkts, touch,
                               ex->hctl + 515, ex->slots, ex->hctl);
            hipLaunchKernelGGL(k_exh_pick, dim3(1), dim3(512), 0, s, ex->hctl, ex->hctl + 512);
            hipLaunchKernelGGL(k_exh_collect_list, dim3(sg), dim3(256), 0, s, ex->f.pkts, touch, ex->hctl + 515,
                               ex->slots, ex->hctl + 512, ex->hctl + 513, ex->hot_ids);
        } else {
            const unsigned sg = (unsigned)((ex->slots + 255) / 256);
            hipLaunchKernelGGL(k_ex_times, dim3(sg), dim3(256), 0, s, ex->f, ex->slots, pos, n, xin.ts);
            GNS_HIP(hipMemsetAsync(ex->hctl, 0, 514 * 4, s));
            GNS_HIP(hipMemsetAsync(ex->hot_ids, 0xFF, kExHot * 4, s));
            hipLaunchKernelGGL(k_exh_hist, dim3(std::min<unsigned>(sg, 2048)), dim3(256), 0, s, ex->f.pkts, ex->slots,
                               ex->hctl);
            hipLaunchKernelGGL(k_exh_pick, dim3(1), dim3(512), 0, s, ex->hctl, ex->hctl + 512);
            hipLaunchKernelGGL(k_exh_collect, dim3(sg), dim3(256), 0, s, ex->f.pkts, ex->slots, ex->hctl + 512,
                               ex->hctl + 513, ex->hot_ids);
        }
        hipLaunchKernelGGL(k_exh_table, dim3(1), dim3(kExHot), 0, s, ex->hot_ids, ex->f.pkts, ex->hot_tab);
        GNS_HIP(hipGetLastError());
    }
    ex->pkt += n;
    ex->batches++;
    ex->warm = true;
    return GNS_OK;
}

// Sort-word fields for the current table: flow ids < slots (invalid packets =
// slots), packet index, wire length (>= 12 bits; a longer length is read back by X3).
int ex_geometry(gns_ex *ex) {
    uint32_t kb = 1;
    while ((1ull << kb) <= ex->slots) kb++;
    ex->key_bits = kb;
    if (64 - kb - ceil_log2(ex->bmax) < 12) ex->bmax = 1ull << (52 - kb);
    ex->nblk_max = (uint32_t)(ex->bmax / kXChunk);
    ex->ib = std::max<uint32_t>(1, ceil_log2(ex->bmax));
    ex->sb = std::min<uint32_t>(31, 64 - kb - ex->ib);
    return GNS_OK;
}

// The exact aggregator keeps every flow of the period (exact/task.go:135-148
// grows a Go map): when the dictionary fills, the table doubles.  Flows with
// packets are reinserted (gns_dict.hip) and their state follows them; the
// claims of an aborted batch (flows without packets yet) are dropped.
// keep_reached (gns_ex_hist_rollup_between): the slots that move are those some row has reached
// (last != 0), not those with packets -- between two pieces of a window a group's packet change
// may stand at 0 with a byte change and times that the next piece's rows still add to.
int ex_grow(gns_ex *ex, bool keep_reached = false) {
    const uint64_t old_slots = ex->slots, new_slots = old_slots * 2;
    if (new_slots > (1ull << 30)) {
        set_error("exact flow dictionary cannot grow beyond 2^30 slots (%llu flows)", (unsigned long long)ex->claimed);
        return GNS_E_FULL;
    }
    const auto t0 = std::chrono::steady_clock::now();
    FlowState nf{};
    int rc = GNS_OK;
    if ((rc = dalloc_t(&nf.pkts, new_slots)) || (rc = dalloc_t(&nf.bytes, new_slots)) ||
        (rc = dalloc_t(&nf.first, new_slots)) || (rc = dalloc_t(&nf.last, new_slots)) ||
        (rc = dalloc_t(&nf.start, new_slots)) || (rc = dalloc_t(&nf.end, new_slots))) {
        dfree(nf.pkts); dfree(nf.bytes); dfree(nf.first); dfree(nf.last); dfree(nf.start); dfree(nf.end);
        return rc;
    }
    uint64_t slots = ex->slots, live = 0;
    rc = dict_rebuild(ex->D, slots, nullptr, 0, keep_reached ? ex->f.last : ex->f.pkts, nullptr, 0, new_slots, ex->stream, ex->dsc, &live, nullptr);
    if (rc != GNS_OK) {
        dfree(nf.pkts); dfree(nf.bytes); dfree(nf.first); dfree(nf.last); dfree(nf.start); dfree(nf.end);
        return rc;
    }
    hipLaunchKernelGGL(k_ex_init, dim3((unsigned)((new_slots + 255) / 256)), dim3(256), 0, ex->stream, nf, new_slots);
    hipLaunchKernelGGL(k_ex_permute, dim3((unsigned)((old_slots + 255) / 256)), dim3(256), 0, ex->stream, ex->f,
                       old_slots, ex->dsc.remap, nf);
    GNS_HIP(hipGetLastError());
    GNS_HIP(hipStreamSynchronize(ex->stream));
    dfree(ex->f.pkts); dfree(ex->f.bytes); dfree(ex->f.first); dfree(ex->f.last); dfree(ex->f.start); dfree(ex->f.end);
    ex->f = nf;
    ex->slots = new_slots;
    ex->D.cap = (uint32_t)(new_slots - new_slots / 4);
    ex->claimed = live;
    GNS_TRY(ex_geometry(ex));
    GNS_TRY(ex_hot_clear(ex));  // designated ids name old slots
    ex->n_grow++;
    ex->grow_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GNS_OK;
}

template <int KIND>
int ex_dispatch(gns_ex *ex, const ExIn &x, uint64_t n) {
    switch (plan_mode(ex->kp)) {
    case PLAN_SLICE0: return ex_run_batch<KIND, PLAN_SLICE0>(ex, x, n);
    case PLAN_SLICE4: return ex_run_batch<KIND, PLAN_SLICE4>(ex, x, n);
    default: return ex_run_batch<KIND, PLAN_GENERIC>(ex, x, n);
    }
}

// One device batch with table growth: a batch that overflows the dictionary is
// aborted before X3 touches the flow state, its counters are undone, the table
// doubles and the batch runs again.
ExIn ex_advance(const ExIn &x0, uint64_t off) {
    ExIn x = x0;
    x.in = advance(x0.in, off);
    if (x.ipver) x.ipver += off;
    x.ts += off;
    return x;
}

template <int KIND>
int ex_batch_recover(gns_ex *ex, const ExIn &x, uint64_t m) {
    if (ex->claimed >= ex->slots / 2) GNS_TRY(ex_grow(ex));  // keep the load <= ~1/2
    if (m > ex->bmax) {  // a grown table leaves fewer sort-word bits for the packet index
        for (uint64_t off = 0; off < m; off += ex->bmax)
            GNS_TRY(ex_batch_recover<KIND>(ex, ex_advance(x, off), std::min<uint64_t>(ex->bmax, m - off)));
        return GNS_OK;
    }
    for (;;) {
        GNS_TRY(stats_save(ex->stats_bak, ex->stats, ex->stream));
        const int rc = ex_dispatch<KIND>(ex, x, m);
        if (rc != GNS_E_FULL) return rc;
        GNS_TRY(stats_undo(ex->stats, ex->stats_bak, true, ex->stream));
        ex->n_retry++;
        const int g = ex_grow(ex);
        if (g != GNS_OK) {
            const unsigned long long one = 1;
            (void)hipMemcpy(ex->stats + 3, &one, sizeof(one), hipMemcpyHostToDevice);
            return g;
        }
        if (m > ex->bmax) return ex_batch_recover<KIND>(ex, x, m);
    }
}

template <int KIND>
int ex_insert(gns_ex *ex, const ExIn &x0, uint64_t n, gns_mem where) {
    GNS_TRY(set_device(ex->device));
    for (uint64_t off = 0, m = 0; off < n; off += m) {
        // a batch without designated flows sends every packet through P (the heavy
        // flows serialise in P4's LDS atomics): keep it short, so that designation
        // starts early (as Count-Min's cold start)
        const uint64_t cap = ex->warm ? ex->bmax : std::min<uint64_t>(ex->bmax, std::max<uint64_t>(1ull << 20, ex->bmax / 32));
        m = std::min<uint64_t>(cap, n - off);
        ExIn x = ex_advance(x0, off);
        if (where != GNS_MEM_DEVICE) {  // stage the piece on the device
            StageList l;
            stage_input(l, x.in, m);
            stage_add(l, x.ipver, x.ipver ? m : 0, &x.ipver);
            stage_add(l, x.ts, m * 8, &x.ts);
            GNS_TRY(ex->stage.copy(l, ex->stream));
        }
        if constexpr (KIND == IN_REC16) GNS_TRY(ex->compact.unpack_sizes(x.in, m, ex->stream));
        GNS_TRY(ex_batch_recover<KIND>(ex, x, m));
    }
    return GNS_OK;
}

// ---------------------------------------------------------------------------
// Read side: the query plane as functions of (table, rows, stream, scratch): the same
// code answers for the live table on the handle's stream and for a view's dense rows on
// the view's own stream.
// ---------------------------------------------------------------------------
// One table the query kernels scan: the live table (rows = slots) or a view's rows.
struct ExTable {
    DictDev D;
    FlowState f;
    uint64_t rows;
};

// A batch of filters as the two public forms hand it over: gns_ex_filter (every masked field
// compared whole) or gns_ex_cidr (the filter first, then the leading bits of the two IP fields
// that take part).  Equality is the 128-bit case.
struct ExFilters {
    const uint8_t *base;
    size_t stride;
    bool cidr;
    ExFilters(const gns_ex_filter *f) : base(reinterpret_cast<const uint8_t *>(f)), stride(sizeof(gns_ex_filter)), cidr(false) {}
    ExFilters(const gns_ex_cidr *f) : base(reinterpret_cast<const uint8_t *>(f)), stride(sizeof(gns_ex_cidr)), cidr(true) {}
    const gns_ex_filter &at(uint32_t i) const { return *reinterpret_cast<const gns_ex_filter *>(base + i * stride); }
    uint32_t bits(uint32_t i, uint32_t fld) const {  // fld: GNS_F_SRCIP or GNS_F_DSTIP
        if (!cidr) return 128;
        const gns_ex_cidr &c = *reinterpret_cast<const gns_ex_cidr *>(base + i * stride);
        return fld == GNS_F_SRCIP ? c.src_bits : c.dst_bits;
    }
};

int ex_filters_check(const ExFilters &filters, uint32_t nf) {
    constexpr uint32_t kFieldBits = (1u << GNS_F_SRCIP) | (1u << GNS_F_DSTIP) | (1u << GNS_F_SRCPORT) |
                                    (1u << GNS_F_DSTPORT) | (1u << GNS_F_PROTO);
    for (uint32_t i = 0; i < nf; i++) {
        if (filters.at(i).mask & ~kFieldBits) {
            set_error("filter %u: mask 0x%x has bits outside the five key fields", i, filters.at(i).mask);
            return GNS_E_ARG;
        }
        if (filters.bits(i, GNS_F_SRCIP) > 128 || filters.bits(i, GNS_F_DSTIP) > 128) {
            set_error("filter %u: prefix of %u / %u bits (0..128 of the 16-byte form)", i, filters.bits(i, GNS_F_SRCIP),
                      filters.bits(i, GNS_F_DSTIP));
            return GNS_E_ARG;
        }
    }
    return GNS_OK;
}

// gns_ex_aggregate over table T (the argument checks are the caller's; nf != 0)
// asof: T is a history's log, answered as of that snapshot
int ex_aggregate_on(const KeyPlanN &kp, const ExTable &T, hipStream_t s, ExRead &rd, StageTimer *timer,
                    const ExFilters &filters, uint32_t nf, gns_ex_summary *out, const ExSelAsOf *asof = nullptr) {
    // per filter: the 37 tuple bytes (make_plan's numbering), which fields are masked and, bit
    // for bit, how much of each byte takes part (an IP field under a prefix: its leading bits);
    // the layout's byte plan carries them to their place in the record's key words
    static const struct { uint32_t base, len; } kSpan[6] = {{0, 0}, {0, 16}, {16, 16}, {32, 2}, {34, 2}, {36, 1}};
    const size_t acc_bytes = (size_t)nf * kQAcc * 8, flt_bytes = (size_t)nf * sizeof(ExQFilter);
    std::vector<ExQFilter> vf;
    std::vector<unsigned long long> va;
    ExQFilter *hf;
    unsigned long long *ha;
    if (rd.keep) {  // staged in the view's pinned buffer: accumulators, then filters
        GNS_TRY(rd.po.reserve(acc_bytes + flt_bytes));
        ha = reinterpret_cast<unsigned long long *>(rd.po.pin);
        hf = reinterpret_cast<ExQFilter *>(rd.po.pin + acc_bytes);
    } else {
        vf.resize(nf);
        va.resize((size_t)nf * kQAcc);
        hf = vf.data();
        ha = va.data();
    }
    for (uint32_t i = 0; i < nf; i++) {
        const gns_ex_filter &q = filters.at(i);
        uint8_t tb[40] = {0}, tm[40] = {0}, want[40] = {0};
        memcpy(tb, q.src16, 16);
        memcpy(tb + 16, q.dst16, 16);
        tb[32] = (uint8_t)(q.sport >> 8); tb[33] = (uint8_t)q.sport;
        tb[34] = (uint8_t)(q.dport >> 8); tb[35] = (uint8_t)q.dport;
        tb[36] = q.proto;
        for (uint32_t fld = GNS_F_SRCIP; fld <= GNS_F_PROTO; fld++)
            if (q.mask >> fld & 1u) {
                memset(want + kSpan[fld].base, 1, kSpan[fld].len);
                const uint32_t bits = fld <= GNS_F_DSTIP ? filters.bits(i, fld) : 8 * kSpan[fld].len;
                for (uint32_t b = 0; b < kSpan[fld].len; b++)
                    tm[kSpan[fld].base + b] = px_prefix_byte(bits, b);
            }
        ExQFilter &w = hf[i];
        memset(&w, 0, sizeof(w));
        uint8_t seen[40] = {0};
        for (uint32_t j = 0; j < kp.K; j++) {
            const uint32_t t = kp.src[j];
            if (t >= 37 || !want[t]) continue;
            seen[t] = 1;
            w.m[j >> 2] |= (uint32_t)tm[t] << (8 * (j & 3));
            w.v[j >> 2] |= (uint32_t)(tb[t] & tm[t]) << (8 * (j & 3));  // address bits below the prefix are ignored
        }
        // a masked field outside the key is a NULL column (writer_clickhouse.go:142-148):
        // `NULL = ?` selects nothing -> a pair no word satisfies
        for (uint32_t t = 0; t < 37; t++)
            if (want[t] && !seen[t]) { w.m[0] = 0u; w.v[0] = 1u; break; }
        for (uint32_t j = 0; j < kQAcc; j++) ha[(size_t)i * kQAcc + j] = exq_acc_init(j);
    }
    if (T.rows != 0) {  // (a view without rows: every answer is the initial one)
        GNS_TRY(rd.buf(&rd.df, rd.df_n, nf));
        GNS_TRY(rd.buf(&rd.da, rd.da_n, (uint64_t)nf * kQAcc));
        ExQFilter *df = rd.df;
        unsigned long long *da = rd.da;
        hipError_t e = hipMemcpyAsync(df, hf, flt_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(da, ha, acc_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            std::optional<ScopedStage> stg;
            if (timer) stg.emplace(*timer, 6);
            const unsigned grid = (unsigned)std::min<uint64_t>((T.rows + 255) / 256, 2048);
            for (uint32_t p0 = 0; p0 < nf; p0 += kQBatch) {
                const uint32_t nb = std::min(kQBatch, nf - p0);
                if (asof && nb > kQNarrow)
                    hipLaunchKernelGGL((k_exq_aggregate<true, ExSelAsOf>), dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, df + p0,
                                       nb, da + (size_t)p0 * kQAcc, *asof);
                else if (asof)
                    hipLaunchKernelGGL((k_exq_aggregate<false, ExSelAsOf>), dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, df + p0,
                                       nb, da + (size_t)p0 * kQAcc, *asof);
                else if (nb > kQNarrow)
                    hipLaunchKernelGGL(k_exq_aggregate<true>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, df + p0,
                                       nb, da + (size_t)p0 * kQAcc);
                else
                    hipLaunchKernelGGL(k_exq_aggregate<false>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, df + p0,
                                       nb, da + (size_t)p0 * kQAcc);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(ha, da, acc_bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("exact aggregate: %s", hipGetErrorString(e)); return GNS_E_HIP; }
    }
    for (uint32_t i = 0; i < nf; i++) {
        const unsigned long long *a = &ha[(size_t)i * kQAcc];
        gns_ex_summary &o = out[i];
        memset(&o, 0, sizeof(o));
        if (a[0] == 0) continue;
        o.flows = a[0]; o.packets = a[1]; o.bytes = a[2];
        o.first_ns = (int64_t)(a[3] ^ kQSign); o.last_ns = (int64_t)(a[4] ^ kQSign);
        o.max_packets = a[5]; o.max_bytes = a[6];
    }
    return GNS_OK;
}

// gns_ex_heavy_hitters over table T (the argument checks are the caller's)
int ex_heavy_on(uint32_t K, const ExTable &T, hipStream_t s, ExRead &rd, StageTimer *timer, int metric,
                uint64_t threshold, uint64_t limit, uint8_t *keys, uint64_t *values, uint64_t *n_io,
                const ExSelAsOf *asof = nullptr, const ExSelSigned *mv = nullptr) {
    if (T.rows == 0) {  // a view without rows
        *n_io = 0;
        return GNS_OK;
    }
    const unsigned grid = (unsigned)std::min<uint64_t>((T.rows + 255) / 256, 2048);
    GNS_TRY(rd.buf(&rd.dh, rd.dh_n, kQBands + 1));  // [0..kQBands) band histogram, [kQBands] rows collected
    uint32_t *dh = rd.dh;
    std::vector<uint32_t> vh;
    uint32_t *hist;
    if (rd.keep) {
        hist = reinterpret_cast<uint32_t *>(rd.po.pin);  // (two chunks of room: never smaller than the histogram)
    } else {
        vh.resize(kQBands);
        hist = vh.data();
    }
    hipError_t e = hipMemsetAsync(dh, 0, (kQBands + 1) * 4, s);
    if (e == hipSuccess) {
        std::optional<ScopedStage> stg;
        if (timer) stg.emplace(*timer, 6);
        if (asof)
            hipLaunchKernelGGL(k_exq_hh_hist<ExSelAsOf>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, metric,
                               (unsigned long long)threshold, dh, *asof);
        else if (mv)
            hipLaunchKernelGGL(k_exq_hh_hist<ExSelSigned>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, metric,
                               (unsigned long long)threshold, dh, *mv);
        else
            hipLaunchKernelGGL(k_exq_hh_hist<>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, metric,
                               (unsigned long long)threshold, dh);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hist, dh, kQBands * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_error("exact heavy hitters: %s", hipGetErrorString(e)); return GNS_E_HIP; }
    uint64_t total = 0;
    for (uint32_t b = 0; b < kQBands; b++) total += hist[b];
    const uint64_t cap = *n_io, len = limit ? std::min<uint64_t>(limit, total) : total;
    *n_io = len;
    if (len == 0 || len > cap || (!keys && !values)) return GNS_OK;
    // the lowest band the first `len` rows can reach, and the rows from it up
    uint32_t band = kQBands - 1;
    uint64_t nrows = hist[band];
    while (band > 0 && nrows < len) nrows += hist[--band];
    size_t tmp_bytes = 0;
    ExHhRow *none = nullptr;
    if (rocprim::merge_sort(nullptr, tmp_bytes, none, none, (size_t)nrows, ExHhLess(), s) != hipSuccess) {
        set_error("exact heavy hitters: merge sort sizing");
        return GNS_E_HIP;
    }
    GNS_TRY(rd.buf(&rd.rows[0], rd.rows_n[0], nrows));
    GNS_TRY(rd.buf(&rd.rows[1], rd.rows_n[1], nrows));
    GNS_TRY(rd.buf(&rd.tmp, rd.tmp_n, tmp_bytes));
    GNS_TRY(rd.buf(&rd.dk, rd.dk_n, len * std::max<uint32_t>(K, 1)));
    GNS_TRY(rd.buf(&rd.dv, rd.dv_n, len));
    {
        std::optional<ScopedStage> stg;
        if (timer) stg.emplace(*timer, 6);
        if (asof)
            hipLaunchKernelGGL(k_exq_hh_collect<ExSelAsOf>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, metric,
                               (unsigned long long)threshold, band, rd.rows[0], dh + kQBands, (uint32_t)nrows, *asof);
        else if (mv)
            hipLaunchKernelGGL(k_exq_hh_collect<ExSelSigned>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, metric,
                               (unsigned long long)threshold, band, rd.rows[0], dh + kQBands, (uint32_t)nrows, *mv);
        else
            hipLaunchKernelGGL(k_exq_hh_collect<>, dim3(grid), dim3(256), 0, s, T.D, T.rows, T.f, metric,
                               (unsigned long long)threshold, band, rd.rows[0], dh + kQBands, (uint32_t)nrows);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = rocprim::merge_sort(rd.tmp, tmp_bytes, rd.rows[0], rd.rows[1], (size_t)nrows, ExHhLess(), s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_exq_hh_out, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, rd.rows[1], len,
                               K, rd.dk, rd.dv);
            if (mv)
                hipLaunchKernelGGL(k_exq_mv_sign, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, rd.rows[1], len,
                                   rd.dv);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) { set_error("exact heavy hitters: %s", hipGetErrorString(e)); return GNS_E_HIP; }
    if (keys) GNS_TRY(rd.copy_out(keys, rd.dk, len * K, s));
    if (values) GNS_TRY(rd.copy_out(values, rd.dv, len * 8, s));
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

// --- snapshot view ---
void exv_free_rows(DictDev &D, FlowState &f) {
    dfree(D.rec); dfree(f.pkts); dfree(f.bytes); dfree(f.start); dfree(f.end);
    D.rec = nullptr;
    f.pkts = f.bytes = nullptr;
    f.start = f.end = nullptr;
}

void exv_free(gns_ex_view *v) {
    exv_free_rows(v->D, v->f);
    dfree(v->scan); dfree(v->total);
    v->rd.free_all();
    v->destroy();
}

// Room for `need` rows.  Growing is an ingest-side matter: new tables first (a failure
// leaves the view as it was), then the old ones are freed, which waits for whatever of an
// earlier refresh is still running on the handle's stream.
int exv_reserve(gns_ex_view *v, uint64_t need) {
    if (need <= v->cap) return GNS_OK;
    const gns_ex *ex = v->ex;
    const uint64_t cap = std::max<uint64_t>(std::min<uint64_t>(2 * need, ex->slots), need);
    DictDev D = v->D;
    FlowState f{};
    D.rec = nullptr;
    int rc;
    if ((rc = dalloc_t(&D.rec, cap * D.RW)) || (rc = dalloc_t(&f.pkts, cap)) || (rc = dalloc_t(&f.bytes, cap)) ||
        (rc = dalloc_t(&f.start, cap)) || (rc = dalloc_t(&f.end, cap))) {
        exv_free_rows(D, f);
        return rc;
    }
    exv_free_rows(v->D, v->f);
    v->D = D;
    v->f = f;
    v->cap = cap;
    return GNS_OK;
}

// reader side, under v->mu: the view has rows to answer from; v->n = their number
int exv_rows(gns_ex_view *v) {
    if (!v->fresh) { set_error("view never refreshed"); return GNS_E_ARG; }
    if (!v->counted) {
        uint32_t *h = reinterpret_cast<uint32_t *>(v->rd.po.pin);
        GNS_HIP(hipMemcpyAsync(h, v->total, 4, hipMemcpyDeviceToHost, v->stream));
        GNS_HIP(hipStreamSynchronize(v->stream));
        v->n = std::min<uint64_t>(*h, v->cap);
        v->counted = true;
    }
    return GNS_OK;
}

// The ids of a piece of m key rows (device memory, <= kResolvePiece; row i is live when
// vals[i] != 0) on ex's table, which grows as the rows need: no state is written before every
// id of the piece is known.  *added, when given, grows by the slots the piece claimed.
int ex_resolve_rows(gns_ex *ex, const uint8_t *keys, uint32_t stride, uint64_t m, const unsigned long long *vals,
                    uint32_t *ids, KeyResolveScratch &sc, uint64_t *added, bool keep_reached = false) {
    hipStream_t s = ex->stream;
    if (ex->claimed >= ex->slots / 2) GNS_TRY(ex_grow(ex, keep_reached));  // keep the load <= ~1/2
    KeyResolve r{};
    r.keys = keys; r.stride = stride; r.n = m; r.live = KEYS_VAL64; r.vals = vals; r.ids = ids;
    r.full_word = ex->stats + 3;
    for (;;) {
        const uint64_t before = ex->claimed;
        const int rc = dict_resolve_keys(ex->D, ex->epoch, r, sc, s, &ex->claimed, &ex->timer, 1);
        if (rc == GNS_OK && added) *added += ex->claimed - before;
        if (rc != GNS_E_FULL) return rc;
        GNS_HIP(hipMemsetAsync(ex->stats + 3, 0, sizeof(unsigned long long), s));
        ex->n_retry++;
        GNS_TRY(ex_grow(ex, keep_reached));  // the state already written follows the table; the piece's claims are dropped
    }
}
}  // namespace

extern "C" {

int gns_ex_create(const gns_ex_params *p, gns_ex **out) {
    if (!p || !out) { set_error("null argument"); return GNS_E_ARG; }
    *out = nullptr;
    GNS_TRY(check_device(p->device));
    gns_ex *ex = new gns_ex();
    ex->device = p->device;
    int rc = GNS_OK;
    do {
        if ((rc = set_device(ex->device)) != GNS_OK) break;
        if (p->key.n_fields == 0) { set_error("exact task needs key_fields"); rc = GNS_E_ARG; break; }
        for (uint32_t i = 0; i < p->key.n_fields; i++)
            if (p->key.fields[i] < GNS_F_SRCIP || p->key.fields[i] > GNS_F_PROTO) {
                set_error("unknown key field id %u (task.go:363 rejects it)", p->key.fields[i]);
                rc = GNS_E_ARG;
            }
        if (rc) break;
        if ((rc = make_plan(p->key, 0, &ex->kp)) != GNS_OK) break;
        ex->K = ex->kp.K;
        if (hipStreamCreateWithFlags(&ex->stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed"); rc = GNS_E_HIP; break;
        }
        ex->timer.stream = ex->stream;
        const uint64_t mf = p->max_flows ? p->max_flows : (4ull << 20);
        uint64_t slots = 1;
        while (slots < 2 * mf) slots <<= 1;
        if (slots > (1ull << 30)) { set_error("max_flows too large"); rc = GNS_E_ARG; break; }
        ex->slots = slots;
        ex->D.mask = (uint32_t)(slots - 1);
        ex->D.K = ex->K;
        ex->D.RW = dict_record_words(ex->K);
        ex->D.seed = 0x5BD1E995u;
        {
            const char *env = getenv("GNS_EX_LIST");
            ex->force_list = env && env[0] == '1';
        }
        ex->bmax = p->batch_packets ? p->batch_packets : (16ull << 20);
        ex->bmax = std::min<uint64_t>(((ex->bmax + kXChunk - 1) / kXChunk) * kXChunk, 1ull << 31);
        {   // sort word fields (ex_geometry, before the batch buffers are sized)
            uint32_t kb = 1;
            while ((1ull << kb) <= slots) kb++;
            if (64 - kb - ceil_log2(ex->bmax) < 12) ex->bmax = 1ull << (52 - kb);
        }
        ex->nblk_max = (uint32_t)(ex->bmax / kXChunk);
        if ((rc = dalloc_t(&ex->D.rec, slots * ex->D.RW)) || (rc = dalloc_t(&ex->f.pkts, slots)) ||
            (rc = dalloc_t(&ex->f.bytes, slots)) || (rc = dalloc_t(&ex->f.first, slots)) ||
            (rc = dalloc_t(&ex->f.last, slots)) || (rc = dalloc_t(&ex->f.start, slots)) ||
            (rc = dalloc_t(&ex->f.end, slots)) ||
            (rc = dalloc_t(&ex->pend[0], ex->bmax)) || (rc = dalloc_t(&ex->pend[1], ex->bmax)) ||
            (rc = dalloc_t(&ex->pcnt[0], ex->nblk_max)) || (rc = dalloc_t(&ex->pcnt[1], ex->nblk_max)) ||
            (rc = dalloc_t(&ex->ptotal, 2)) || (rc = dalloc_t(&ex->stats, 8)) ||
            (rc = dalloc_t(&ex->sk[0], ex->bmax)) || (rc = dalloc_t(&ex->sk[1], ex->bmax)) ||
            (rc = dalloc_t(&ex->hot_ids, kExHot)) || (rc = dalloc_t(&ex->touch, ex->bmax + kExHot)) || (rc = dalloc_t(&ex->hot_tab, kExHotTab)) ||
            (rc = dalloc_t(&ex->hpart, (uint64_t)kExHot * ex->nblk_max)) || (rc = dalloc_t(&ex->hctl, 516)) ||
            (rc = dalloc_t(&ex->ccnt, ex->nblk_max)) || (rc = dalloc_t(&ex->ph, (uint64_t)ex->nblk_max * kPBins)) ||
            (rc = dalloc_t(&ex->pgs, (uint64_t)(ex->nblk_max / kPGroup + 1) * kPBins)) ||
            (rc = dalloc_t(&ex->pb, kPBins + 1)))
            break;
        if ((rc = ex_geometry(ex)) != GNS_OK) break;
        if ((rc = dalloc_t(&ex->dctl, 4)) != GNS_OK || (rc = dalloc_t(&ex->stats_bak, 3)) != GNS_OK) break;
        ex->D.ctl = ex->dctl;
        ex->D.cap = (uint32_t)(slots - slots / 4);
        if (hipHostMalloc(reinterpret_cast<void **>(&ex->h_pin), 64, 0) != hipSuccess) {
            set_error("hipHostMalloc failed"); rc = GNS_E_OOM; break;
        }
        if (hipMemsetAsync(ex->stats, 0, 64, ex->stream) != hipSuccess) { rc = GNS_E_HIP; break; }
        if ((rc = ex_clear(ex)) != GNS_OK) break;
        if (hipStreamSynchronize(ex->stream) != hipSuccess) { rc = GNS_E_HIP; break; }
    } while (0);
    if (rc != GNS_OK) {
        ex_free_all(ex);
        delete ex;
        return rc;
    }
    *out = ex;
    return GNS_OK;
}

int gns_ex_destroy(gns_ex *ex) {
    if (!ex) return GNS_OK;
    (void)hipSetDevice(ex->device);
    if (ex->stream) (void)hipStreamSynchronize(ex->stream);
    ex_free_all(ex);
    delete ex;
    return GNS_OK;
}

int gns_ex_insert_tuples(gns_ex *ex, const gns_tuples *t, const uint8_t *ipver, const int64_t *ts_ns,
                         uint64_t n, gns_mem where) {
    if (!ex || !t) { set_error("null argument"); return GNS_E_ARG; }
    if (n && (!t->src16 || !t->dst16 || !t->sport || !t->dport || !t->proto || !t->length || !ts_ns)) {
        set_error("null tuple array"); return GNS_E_ARG;
    }
    ExIn x{};
    x.in = tuples_desc(*t, true);
    x.ipver = ipver; x.ts = ts_ns;
    return ex_insert<IN_TUPLE>(ex, x, n, where);
}

int gns_ex_insert_headers(gns_ex *ex, const uint8_t *hdr, const uint32_t *wirelen, const int64_t *ts_ns,
                          uint64_t n, gns_mem where) {
    if (!ex || (n && (!hdr || !wirelen || !ts_ns))) { set_error("null argument"); return GNS_E_ARG; }
    ExIn x{};
    x.in = headers_desc(hdr, wirelen);
    x.ts = ts_ns;
    return ex_insert<IN_HDR>(ex, x, n, where);
}

int gns_ex_insert_compact(gns_ex *ex, const uint8_t *rec16, const uint32_t *wirelen, const int64_t *ts_ns,
                          uint64_t n, const uint8_t *side64, uint64_t n_side, gns_mem where) {
    if (!ex || !ts_ns || (n && !rec16) || (n_side && !side64)) { set_error("null argument"); return GNS_E_ARG; }
    ExIn x{};
    x.in = compact_desc(rec16, wirelen, side64, n_side);
    x.ts = ts_ns;
    if (where != GNS_MEM_DEVICE) {  // the resolve rounds re-read the side records: one device copy for the whole call
        GNS_TRY(set_device(ex->device));
        GNS_TRY(ex->compact.stage_side(x.in, ex->stream));
    }
    return ex_insert<IN_REC16>(ex, x, n, where);
}

int gns_ex_flush(gns_ex *ex) {
    if (!ex) return GNS_E_ARG;
    return handle_flush(ex->device, ex->stream, ex->timer);
}

static int ex_query_impl(gns_ex *ex, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out, bool dev) {
    if (!ex) { set_error("null argument"); return GNS_E_ARG; }
    return query_keys(ex->device, ex->stream, ex->qs, "exact", flows, stride, ex->K, n, out, dev,
                      [&](const uint8_t *dk, uint64_t *dout) -> int {
                          hipLaunchKernelGGL(k_ex_query, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ex->stream, dk,
                                             stride, n, ex->K, ex->D, ex->f, dout);
                          return GNS_OK;
                      });
}

int gns_ex_query(gns_ex *ex, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out) {
    return ex_query_impl(ex, flows, stride, n, out, false);
}

int gns_ex_query_device(gns_ex *ex, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out) {
    return ex_query_impl(ex, flows, stride, n, out, true);
}

int gns_ex_snapshot(gns_ex *ex, uint8_t *keys, int64_t *start_ns, int64_t *end_ns, uint64_t *pkts,
                    uint64_t *bytes, uint64_t *n_io) {
    if (!ex || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(ex->device));
    hipStream_t s = ex->stream;
    uint32_t *ids = nullptr, *cnt = nullptr;
    GNS_TRY(dalloc(reinterpret_cast<void **>(&cnt), 16));
    int rc = dalloc(reinterpret_cast<void **>(&ids), ex->slots * 4);
    if (rc) { dfree(cnt); return rc; }
    uint32_t nf = 0;
    hipError_t e = hipMemsetAsync(cnt, 0, 4, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_ex_list, dim3((unsigned)((ex->slots + 255) / 256)), dim3(256), 0, s, ex->D, ex->slots,
                           ex->f.pkts, ids, cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&nf, cnt, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const uint64_t cap = *n_io;
    *n_io = nf;
    const uint64_t m = std::min<uint64_t>(cap, nf);
    if (e == hipSuccess && m > 0 && (keys || start_ns || end_ns || pkts || bytes)) {
        // slot order (deterministic)
        std::vector<uint32_t> h(nf);
        e = hipMemcpy(h.data(), ids, (size_t)nf * 4, hipMemcpyDeviceToHost);
        std::sort(h.begin(), h.end());
        if (e == hipSuccess) e = hipMemcpy(ids, h.data(), (size_t)m * 4, hipMemcpyHostToDevice);
        uint8_t *dk = nullptr;
        long long *ds = nullptr, *de = nullptr;
        unsigned long long *dp = nullptr, *db = nullptr;
        const size_t kb = (size_t)m * std::max<uint32_t>(ex->K, 1);
        if (e == hipSuccess && (dalloc(reinterpret_cast<void **>(&dk), kb) || dalloc_t(&ds, m) || dalloc_t(&de, m) ||
                                dalloc_t(&dp, m) || dalloc_t(&db, m)))
            e = hipErrorOutOfMemory;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_ex_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, ids, m, ex->D, ex->f,
                               dk, ds, de, dp, db);
            e = hipGetLastError();
        }
        if (e == hipSuccess && keys) e = hipMemcpyAsync(keys, dk, (size_t)m * ex->K, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && start_ns) e = hipMemcpyAsync(start_ns, ds, m * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && end_ns) e = hipMemcpyAsync(end_ns, de, m * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && pkts) e = hipMemcpyAsync(pkts, dp, m * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(bytes, db, m * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        dfree(dk); dfree(ds); dfree(de); dfree(dp); dfree(db);
    }
    dfree(ids);
    dfree(cnt);
    if (e != hipSuccess) { set_error("exact snapshot: %s", hipGetErrorString(e)); return GNS_E_HIP; }
    return GNS_OK;
}

namespace {
static int ex_aggregate(gns_ex *ex, const ExFilters &filters, uint32_t nf, gns_ex_summary *out) {
    if (!ex || (nf && (!filters.base || !out))) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(ex_filters_check(filters, nf));
    if (nf == 0) return GNS_OK;
    GNS_TRY(set_device(ex->device));
    ExRead rd;
    const int rc = ex_aggregate_on(ex->kp, ExTable{ex->D, ex->f, ex->slots}, ex->stream, rd, &ex->timer, filters, nf, out);
    rd.free_all();
    return rc;
}
}  // namespace

int gns_ex_aggregate(gns_ex *ex, const gns_ex_filter *filters, uint32_t nf, gns_ex_summary *out) {
    return ex_aggregate(ex, ExFilters(filters), nf, out);
}

int gns_ex_aggregate_cidr(gns_ex *ex, const gns_ex_cidr *filters, uint32_t nf, gns_ex_summary *out) {
    return ex_aggregate(ex, ExFilters(filters), nf, out);
}

int gns_ex_heavy_hitters(gns_ex *ex, int metric, uint64_t threshold, uint64_t limit, uint8_t *keys,
                         uint64_t *values, uint64_t *n_io) {
    if (!ex || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    if (metric != 0 && metric != 1) { set_error("metric %d (0: PacketCount, 1: ByteCount)", metric); return GNS_E_ARG; }
    GNS_TRY(set_device(ex->device));
    ExRead rd;
    const int rc = ex_heavy_on(ex->K, ExTable{ex->D, ex->f, ex->slots}, ex->stream, rd, &ex->timer, metric, threshold,
                               limit, keys, values, n_io);
    rd.free_all();
    return rc;
}

int gns_ex_movers(gns_ex *ex, int metric, int direction, uint64_t threshold, uint64_t limit, uint8_t *keys,
                  int64_t *values, uint64_t *n_io) {
    if (!ex || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    if (metric != 0 && metric != 1) { set_error("metric %d (0: PacketCount, 1: ByteCount)", metric); return GNS_E_ARG; }
    if (direction < -1 || direction > 1) {
        set_error("movers: direction %d (+1: increases, -1: decreases, 0: either)", direction);
        return GNS_E_ARG;
    }
    GNS_TRY(set_device(ex->device));
    ExRead rd;
    const ExSelSigned mv{direction};
    const int rc = ex_heavy_on(ex->K, ExTable{ex->D, ex->f, ex->slots}, ex->stream, rd, &ex->timer, metric,
                               std::max<uint64_t>(threshold, 1), limit, keys, reinterpret_cast<uint64_t *>(values), n_io,
                               nullptr, &mv);
    rd.free_all();
    return rc;
}

// ---------------------------------------------------------------------------
// Snapshot views: the table, or the flows touched since a cursor, exported and
// queried on another thread while the handle ingests (the reference's snapshotter
// hands every flow to the writer while the workers insert, manager.go:139-159,
// exact/task.go:154-194).
// ---------------------------------------------------------------------------
int gns_ex_view_create(gns_ex *ex, gns_ex_view **out) {
    if (!ex || !out) { set_error("null argument"); return GNS_E_ARG; }
    *out = nullptr;
    GNS_TRY(set_device(ex->device));
    gns_ex_view *v = new gns_ex_view();
    v->ex = ex;
    v->D = ex->D;  // RW, K: the record layout; the rest names nothing of the handle's
    v->D.rec = nullptr; v->D.ctl = nullptr; v->D.mask = 0; v->D.cap = 0;
    int rc = GNS_OK;
    do {
        if ((rc = v->init()) != GNS_OK) break;
        if ((rc = v->rd.init_keep()) != GNS_OK || (rc = dalloc_t(&v->total, 4)) != GNS_OK) break;
    } while (0);
    if (rc) { exv_free(v); delete v; return rc; }
    *out = v;
    return GNS_OK;
}

int gns_ex_view_destroy(gns_ex_view *v) {
    if (!v) return GNS_OK;
    (void)hipSetDevice(v->ex->device);
    // a reader call in progress; the mutex is released before the delete (freeing the tables
    // waits for a refresh still running on the handle's stream)
    v->quiesce();
    exv_free(v);
    delete v;
    return GNS_OK;
}

int gns_ex_view_refresh(gns_ex_view *v, uint64_t since, uint64_t *cursor) {
    if (!v) { set_error("null argument"); return GNS_E_ARG; }
    gns_ex *ex = v->ex;
    const uint64_t pos = ex->pkt + ex->merged;  // the next stream position (ex_run_batch, gns_ex_merge)
    if (since > pos) {
        set_error("view refresh: since %llu is beyond the stream position %llu", (unsigned long long)since,
                  (unsigned long long)pos);
        return GNS_E_ARG;
    }
    GNS_TRY(set_device(ex->device));
    std::lock_guard<std::mutex> lk(v->mu);  // no reader is using the rows
    GNS_TRY(exv_reserve(v, std::max<uint64_t>(ex->claimed, 1)));  // rows <= flows with packets <= claimed slots
    const uint32_t nblk = (uint32_t)((ex->slots + 255) / 256);
    const uint32_t nb = (nblk + kVBins - 1) / kVBins, ngrp = (nb + kTGrp - 1) / kTGrp;
    const uint64_t words = (uint64_t)nb * kVBins + (uint64_t)ngrp * kVBins + kVBins;
    if (words > v->scan_n) GNS_TRY(grow_buf(&v->scan, v->scan_n, words));
    uint32_t *cnt = v->scan, *part = cnt + (uint64_t)nb * kVBins, *tot = part + (uint64_t)ngrp * kVBins;
    hipStream_t s = ex->stream;
    v->fresh = false;
    {
        ScopedStage st(ex->timer, 7);
        hipLaunchKernelGGL(k_exv_count, dim3(nb * kVBins), dim3(256), 0, s, ex->D, ex->slots, ex->f,
                           (unsigned long long)since, nb, cnt);
        hipLaunchKernelGGL(k_tscan_part, dim3(1, ngrp), dim3(256), 0, s, cnt, nb, kVBins, part);
        hipLaunchKernelGGL(k_tscan_mid, dim3(1), dim3(256), 0, s, part, ngrp, kVBins, tot);
        hipLaunchKernelGGL(k_tscan_bins, dim3(1), dim3(1024), 0, s, tot, kVBins, v->total);
        hipLaunchKernelGGL(k_tscan_down, dim3(1, ngrp), dim3(256), 0, s, cnt, nb, kVBins, part, tot);
        hipLaunchKernelGGL(k_exv_write, dim3(nblk), dim3(256), 0, s, ex->D, ex->slots, ex->f,
                           (unsigned long long)since, nb, cnt, v->D, v->f, v->cap);
        GNS_HIP(hipGetLastError());
    }
    // the rows are the state after every insert and merge issued so far and before any
    // later one; the view's stream waits for them
    GNS_TRY(v->publish(s));
    v->fresh = true;
    v->counted = false;
    if (cursor) *cursor = pos;
    return GNS_OK;
}

int gns_ex_view_snapshot(gns_ex_view *v, uint8_t *keys, int64_t *start_ns, int64_t *end_ns, uint64_t *pkts,
                         uint64_t *bytes, uint64_t *n_io) {
    if (!v || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(v->ex->device));
    std::lock_guard<std::mutex> lk(v->mu);
    GNS_TRY(exv_rows(v));
    const uint64_t m = std::min<uint64_t>(*n_io, v->n);
    *n_io = v->n;
    if (m == 0) return GNS_OK;
    hipStream_t s = v->stream;
    ExRead &rd = v->rd;
    const uint32_t K = v->ex->K;
    if (keys) {
        GNS_TRY(rd.buf(&rd.dk, rd.dk_n, m * K));
        hipLaunchKernelGGL(k_ex_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const uint32_t *)nullptr, m,
                           v->D, v->f, rd.dk, (long long *)nullptr, (long long *)nullptr,
                           (unsigned long long *)nullptr, (unsigned long long *)nullptr);
        GNS_HIP(hipGetLastError());
        GNS_TRY(rd.copy_out(keys, rd.dk, m * K, s));
    }
    if (start_ns) GNS_TRY(rd.copy_out(start_ns, v->f.start, m * 8, s));
    if (end_ns) GNS_TRY(rd.copy_out(end_ns, v->f.end, m * 8, s));
    if (pkts) GNS_TRY(rd.copy_out(pkts, v->f.pkts, m * 8, s));
    if (bytes) GNS_TRY(rd.copy_out(bytes, v->f.bytes, m * 8, s));
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

namespace {
static int exv_aggregate(gns_ex_view *v, const ExFilters &filters, uint32_t nf, gns_ex_summary *out) {
    if (!v || (nf && (!filters.base || !out))) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(ex_filters_check(filters, nf));
    GNS_TRY(set_device(v->ex->device));
    std::lock_guard<std::mutex> lk(v->mu);
    GNS_TRY(exv_rows(v));
    if (nf == 0) return GNS_OK;
    return ex_aggregate_on(v->ex->kp, ExTable{v->D, v->f, v->n}, v->stream, v->rd, nullptr, filters, nf, out);
}
}  // namespace

int gns_ex_view_aggregate(gns_ex_view *v, const gns_ex_filter *filters, uint32_t nf, gns_ex_summary *out) {
    return exv_aggregate(v, ExFilters(filters), nf, out);
}

int gns_ex_view_aggregate_cidr(gns_ex_view *v, const gns_ex_cidr *filters, uint32_t nf, gns_ex_summary *out) {
    return exv_aggregate(v, ExFilters(filters), nf, out);
}

int gns_ex_view_heavy_hitters(gns_ex_view *v, int metric, uint64_t threshold, uint64_t limit, uint8_t *keys,
                              uint64_t *values, uint64_t *n_io) {
    if (!v || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    if (metric != 0 && metric != 1) { set_error("metric %d (0: PacketCount, 1: ByteCount)", metric); return GNS_E_ARG; }
    GNS_TRY(set_device(v->ex->device));
    std::lock_guard<std::mutex> lk(v->mu);
    GNS_TRY(exv_rows(v));
    return ex_heavy_on(v->ex->K, ExTable{v->D, v->f, v->n}, v->stream, v->rd, nullptr, metric, threshold, limit, keys,
                       values, n_io);
}

// ---------------------------------------------------------------------------
// History: the store behind the Querier's EndTime (`Timestamp <= ?`, querier.go:211-213,
// 271-273, 344-346): every interval's view appended under one timestamp (manager.go:139-159),
// every query answered as of the newest snapshot at or before its end time.
// ---------------------------------------------------------------------------
namespace {
void exh_free_log(ExHistLog &g) {
    dfree(g.L.rec); dfree(g.f.pkts); dfree(g.f.bytes); dfree(g.f.start); dfree(g.f.end);
    dfree(g.written); dfree(g.superseded);
    g.L.rec = nullptr;
    g.f = FlowState{};
    g.written = g.superseded = nullptr;
    g.cap = 0;
}

void exh_free(gns_ex_hist *h) {
    exh_free_log(h->log);
    exv_free_rows(h->SD, h->sf);
    h->ix.free_all();
    dfree(h->head); dfree(h->scan); dfree(h->total);
    h->rd.free_all();
    h->destroy();
}

// An empty log of the history's record layout with room for cap rows (cap == 0: no memory).
int exh_alloc_log(const gns_ex_hist *h, uint64_t cap, ExHistLog *out) {
    const uint32_t RW = h->log.L.RW;
    ExHistLog g = h->log;
    g.L.rec = nullptr;
    g.f = FlowState{};
    g.written = g.superseded = nullptr;
    g.cap = cap;
    int rc;
    if (cap && ((rc = dalloc_t(&g.L.rec, cap * RW)) || (rc = dalloc_t(&g.f.pkts, cap)) || (rc = dalloc_t(&g.f.bytes, cap)) ||
                (rc = dalloc_t(&g.f.start, cap)) || (rc = dalloc_t(&g.f.end, cap)) || (rc = dalloc_t(&g.written, cap)) ||
                (rc = dalloc_t(&g.superseded, cap)))) {
        exh_free_log(g);
        return rc;
    }
    *out = g;
    return GNS_OK;
}

// Room for `need` log rows: allocate, copy the published rows, free (before an append links anything).
int exh_reserve_log(gns_ex_hist *h, uint64_t need) {
    if (need <= h->log.cap) return GNS_OK;
    const uint64_t cap = hist_row_capacity(h->log.cap, need), rows = h->plan.rows;
    const uint32_t RW = h->log.L.RW;
    ExHistLog g;
    GNS_TRY(exh_alloc_log(h, cap, &g));
    hipError_t e = hipSuccess;
    if (rows) {
        hipStream_t s = h->stream;
        const ExHistLog &o = h->log;
        e = hipMemcpyAsync(g.L.rec, o.L.rec, rows * RW * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g.f.pkts, o.f.pkts, rows * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g.f.bytes, o.f.bytes, rows * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g.f.start, o.f.start, rows * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g.f.end, o.f.end, rows * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g.written, o.written, rows * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(g.superseded, o.superseded, rows * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) {
        exh_free_log(g);
        set_error("history log growth: %s", hipGetErrorString(e));
        return GNS_E_HIP;
    }
    if (h->log.cap) h->n_log_grow++;
    exh_free_log(h->log);
    h->log = g;
    return GNS_OK;
}

// A1: ix.ids[i] = the index slot of key i (device, n keys at `stride` bytes).  A growth keeps the
// keys of the published snapshots (a head word) and the ids resolved so far; m != 0: room for a
// piece of m keys if every one of them is new.
int exh_slots_of(gns_ex_hist *h, const uint8_t *keys, uint32_t stride, uint64_t n) {
    hipStream_t s = h->stream;
    return h->ix.resolve(keys, stride, n, 0, s, [&](uint64_t m, uint64_t done) {
        const uint64_t want = m ? h->ix.room_for(h->keys + done + m) : 0;
        if (h->ix.grown(want) > kDictMaxSlots) {
            set_error("history key index cannot grow beyond 2^30 slots (%llu keys)", (unsigned long long)h->keys);
            return (int)GNS_E_FULL;
        }
        return h->ix.grow(want, done, {&h->head}, s);
    });
}

// V1 / V2 over the first `rows` log rows: cnt[exv_cell(block)] = the rank of the block's first
// row among those live under sel, *live the number of them.  Synchronizes the stream.
int exh_rank(gns_ex_hist *h, const ExTable &T, const ExSelAsOf &sel, uint32_t *nb_out, uint64_t *live) {
    hipStream_t s = h->stream;
    const uint32_t nblk = (uint32_t)((T.rows + 255) / 256);
    const uint32_t nb = (nblk + kVBins - 1) / kVBins, ngrp = (nb + kTGrp - 1) / kTGrp;
    const uint64_t words = (uint64_t)nb * kVBins + (uint64_t)ngrp * kVBins + kVBins;
    if (words > h->scan_n) GNS_TRY(grow_buf(&h->scan, h->scan_n, words));
    uint32_t *cnt = h->scan, *part = cnt + (uint64_t)nb * kVBins, *tot = part + (uint64_t)ngrp * kVBins;
    hipLaunchKernelGGL(k_exhv_count, dim3(nb * kVBins), dim3(256), 0, s, T.D, T.rows, T.f, sel, nb, cnt);
    hipLaunchKernelGGL(k_tscan_part, dim3(1, ngrp), dim3(256), 0, s, cnt, nb, kVBins, part);
    hipLaunchKernelGGL(k_tscan_mid, dim3(1), dim3(256), 0, s, part, ngrp, kVBins, tot);
    hipLaunchKernelGGL(k_tscan_bins, dim3(1), dim3(1024), 0, s, tot, kVBins, h->total);
    hipLaunchKernelGGL(k_tscan_down, dim3(1, ngrp), dim3(256), 0, s, cnt, nb, kVBins, part, tot);
    GNS_HIP(hipGetLastError());
    uint32_t *hp = reinterpret_cast<uint32_t *>(h->rd.po.pin);
    GNS_HIP(hipMemcpyAsync(hp, h->total, 4, hipMemcpyDeviceToHost, s));
    GNS_HIP(hipStreamSynchronize(s));
    *nb_out = nb;
    *live = *hp;
    return GNS_OK;
}

// query side, under h->mu: the snapshot a query as of *end_ns sees (-1: none) and its policy
int64_t exh_as_of(const gns_ex_hist *h, const int64_t *end_ns, ExSelAsOf *sel, ExTable *T) {
    const int64_t s = h->plan.as_of(end_ns);
    sel->written = h->log.written;
    sel->superseded = h->log.superseded;
    sel->s = s < 0 ? 0u : (uint32_t)s;
    *T = ExTable{h->log.L, h->log.f, h->plan.rows_as_of(s)};
    return s;
}

int exh_aggregate(gns_ex_hist *h, const int64_t *end_ns, const ExFilters &filters, uint32_t nf, gns_ex_summary *out) {
    if (!h || (nf && (!filters.base || !out))) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(ex_filters_check(filters, nf));
    if (nf == 0) return GNS_OK;
    GNS_TRY(set_device(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    ExSelAsOf sel;
    ExTable T;
    (void)exh_as_of(h, end_ns, &sel, &T);  // (no snapshot: no rows, every answer is the initial one)
    return ex_aggregate_on(h->kp, T, h->stream, h->rd, nullptr, filters, nf, out, &sel);
}
}  // namespace

int gns_ex_hist_create(const gns_ex_hist_params *p, gns_ex_hist **out) {
    if (!p || !out) { set_error("null argument"); return GNS_E_ARG; }
    *out = nullptr;
    GNS_TRY(check_device(p->device));
    if (p->key.n_fields == 0) { set_error("history needs key fields"); return GNS_E_ARG; }
    for (uint32_t i = 0; i < p->key.n_fields; i++)
        if (p->key.fields[i] < GNS_F_SRCIP || p->key.fields[i] > GNS_F_PROTO) {
            set_error("unknown key field id %u (task.go:363 rejects it)", p->key.fields[i]);
            return GNS_E_ARG;
        }
    if (p->max_rows > kHistMax || p->max_flows > kDictMaxSlots / 2) { set_error("history capacity too large"); return GNS_E_ARG; }
    gns_ex_hist *h = new gns_ex_hist();
    h->device = p->device;
    int rc = GNS_OK;
    do {
        if ((rc = set_device(h->device)) != GNS_OK) break;
        if ((rc = make_plan(p->key, 0, &h->kp)) != GNS_OK) break;
        h->K = h->kp.K;
        if ((rc = h->init()) != GNS_OK || (rc = h->rd.init_keep()) != GNS_OK) break;
        const uint64_t slots = hist_index_slots(p->max_flows ? p->max_flows : (64ull << 10));
        if ((rc = dalloc_t(&h->head, slots)) || (rc = dalloc_t(&h->total, 4))) break;
        if (hipMemsetAsync(h->head, 0xFF, slots * 4, h->stream) != hipSuccess) {
            set_error("history create: device clear failed");
            rc = GNS_E_HIP;
            break;
        }
        if ((rc = h->ix.init("history", h->K, slots, h->stream)) != GNS_OK) break;  // (waits for the head words' clear too)
        h->log.L = h->ix.D;
        h->log.L.rec = nullptr; h->log.L.ctl = nullptr; h->log.L.mask = 0; h->log.L.cap = 0;
        h->SD = h->log.L;
        rc = exh_reserve_log(h, p->max_rows ? p->max_rows : (1ull << 20));
    } while (0);
    if (rc != GNS_OK) { exh_free(h); delete h; return rc; }
    *out = h;
    return GNS_OK;
}

int gns_ex_hist_destroy(gns_ex_hist *h) {
    if (!h) return GNS_OK;
    (void)hipSetDevice(h->device);
    h->quiesce();
    exh_free(h);
    delete h;
    return GNS_OK;
}

int gns_ex_hist_append(gns_ex_hist *h, gns_ex_view *v, int64_t timestamp_ns, uint64_t out[2]) {
    if (!h || !v) { set_error("null argument"); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    std::lock_guard<std::mutex> lv(v->mu);  // a reader call on the view: a refresh waits for the append
    if (!v->fresh) { set_error("history append: view never refreshed"); return GNS_E_ARG; }
    if (!hist_same_layout(h->kp.src, h->kp.K, v->ex->kp.src, v->ex->kp.K)) {
        set_error("history append: the view's key layout (%u bytes) is not the history's (%u bytes)", v->ex->kp.K, h->kp.K);
        return GNS_E_ARG;
    }
    if (v->ex->device != h->device) {
        set_error("history append: the view is on device %d, the history on device %d", v->ex->device, h->device);
        return GNS_E_ARG;
    }
    int chk = h->plan.append_check(timestamp_ns, 0);
    if (chk == HIST_E_TIME) {
        set_error("history append: timestamp %lld is not after the last snapshot's %lld", (long long)timestamp_ns,
                  (long long)h->plan.ts.back());
        return GNS_E_ARG;
    }
    if (chk != HIST_OK) { set_error("history holds 2^32 - 2 snapshots"); return GNS_E_FULL; }
    GNS_TRY(set_device(h->device));
    GNS_TRY(exv_rows(v));
    const uint64_t n = v->n;
    if (h->plan.append_check(timestamp_ns, n) != HIST_OK) {
        set_error("history log cannot grow beyond 2^32 - 2 rows (%llu held, %llu appended)", (unsigned long long)h->plan.rows,
                  (unsigned long long)n);
        return GNS_E_FULL;
    }
    hipStream_t s = h->stream;
    const uint32_t S = (uint32_t)h->plan.ts.size();
    uint64_t fresh = 0;
    if (n) {
        GNS_TRY(exh_reserve_log(h, h->plan.rows + n));
        HistIndex &ix = h->ix;
        if (ix.ids_n < n) GNS_TRY(grow_buf(&ix.ids, ix.ids_n, n));
        GNS_TRY(stream_wait_now(s, v->stream, "history append"));  // behind the refresh the view answers for
        // A1 (key words follow the tag)
        GNS_TRY(exh_slots_of(h, reinterpret_cast<const uint8_t *>(v->D.rec + 1), 4 * v->D.RW, n));
        // A2
        GNS_HIP(hipMemsetAsync(ix.fresh, 0, 4, s));
        hipLaunchKernelGGL(k_exh_link, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v->D, v->f, n, ix.ids, h->head,
                           (uint32_t)ix.slots, h->log, h->plan.rows, S, ix.fresh);
        GNS_HIP(hipGetLastError());
        uint32_t *hp = reinterpret_cast<uint32_t *>(h->rd.po.pin);
        GNS_HIP(hipMemcpyAsync(hp, ix.fresh, 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));  // the view's rows are read: a refresh may replace them
        fresh = *hp;
    }
    h->keys += fresh;
    h->plan.publish(timestamp_ns, n);  // last: the snapshot exists from here on
    if (out) { out[0] = n; out[1] = fresh; }
    return GNS_OK;
}

int gns_ex_hist_append_rows(gns_ex_hist *h, const uint8_t *keys, const int64_t *start_ns, const int64_t *end_ns,
                            const uint64_t *pkts, const uint64_t *bytes, uint64_t n, int64_t timestamp_ns,
                            uint64_t out[2]) {
    if (!h || (n && (!keys || !start_ns || !end_ns || !pkts || !bytes))) { set_error("null argument"); return GNS_E_ARG; }
    for (uint64_t i = 0; i < n; i++)
        if (pkts[i] == 0) {
            set_error("history append: row %llu has no packets", (unsigned long long)i);
            return GNS_E_ARG;
        }
    std::lock_guard<std::mutex> lk(h->mu);
    const int chk = h->plan.append_check(timestamp_ns, n);
    if (chk == HIST_E_TIME) {
        set_error("history append: timestamp %lld is not after the last snapshot's %lld", (long long)timestamp_ns,
                  (long long)h->plan.ts.back());
        return GNS_E_ARG;
    }
    if (chk == HIST_E_SNAPSHOTS) { set_error("history holds 2^32 - 2 snapshots"); return GNS_E_FULL; }
    if (chk != HIST_OK) {
        set_error("history log cannot grow beyond 2^32 - 2 rows (%llu held, %llu appended)", (unsigned long long)h->plan.rows,
                  (unsigned long long)n);
        return GNS_E_FULL;
    }
    GNS_TRY(set_device(h->device));
    hipStream_t s = h->stream;
    const uint32_t S = (uint32_t)h->plan.ts.size();
    const uint64_t base = h->plan.rows;
    uint64_t fresh = 0;
    if (n) {
        HistIndex &ix = h->ix;
        if (ix.ids_n < n) GNS_TRY(grow_buf(&ix.ids, ix.ids_n, n));
        ExRead &rd = h->rd;
        PinnedOut &po = rd.po;
        GNS_TRY(rd.buf(&rd.dk, rd.dk_n, n * h->K));
        GNS_TRY(po.copy_in(rd.dk, keys, n * h->K, s));
        GNS_TRY(exh_slots_of(h, rd.dk, h->K, n));
        // no two rows of the call in one index slot, decided before anything is linked
        uint32_t *hp = reinterpret_cast<uint32_t *>(po.pin);
        GNS_HIP(hipMemsetAsync(ix.fresh, 0, 8, s));
        GNS_TRY(ix.check_unique(ix.ids, n, ix.fresh + 1, s));
        GNS_HIP(hipMemcpyAsync(hp, ix.fresh + 1, 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));
        if (*hp) { set_error("history append: two rows of the call have the same key"); return GNS_E_ARG; }
        // the state words go straight behind the published rows, which no query scans
        GNS_TRY(exh_reserve_log(h, base + n));
        GNS_TRY(po.copy_in(h->log.f.start + base, start_ns, n * 8, s));
        GNS_TRY(po.copy_in(h->log.f.end + base, end_ns, n * 8, s));
        GNS_TRY(po.copy_in(h->log.f.pkts + base, pkts, n * 8, s));
        GNS_TRY(po.copy_in(h->log.f.bytes + base, bytes, n * 8, s));
        // A2
        hipLaunchKernelGGL(k_exh_link_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ix.D, n, ix.ids, h->head,
                           (uint32_t)ix.slots, h->log, base, S, ix.fresh);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipMemcpyAsync(hp, ix.fresh, 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));
        fresh = *hp;
    }
    h->keys += fresh;
    h->plan.publish(timestamp_ns, n);  // last: the snapshot exists from here on
    if (out) { out[0] = n; out[1] = fresh; }
    return GNS_OK;
}

int gns_ex_hist_export(gns_ex_hist *h, uint8_t *keys, int64_t *start_ns, int64_t *end_ns, uint64_t *pkts,
                       uint64_t *bytes, uint32_t *written, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t rows = h->plan.rows, m = std::min<uint64_t>(*n_io, rows);
    *n_io = rows;
    if (m == 0 || !(keys || start_ns || end_ns || pkts || bytes || written)) return GNS_OK;
    hipStream_t s = h->stream;
    ExRead &rd = h->rd;
    const ExHistLog &g = h->log;
    if (keys) {  // every published row, in log order
        GNS_TRY(rd.buf(&rd.dk, rd.dk_n, m * h->K));
        hipLaunchKernelGGL(k_ex_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const uint32_t *)nullptr, m,
                           g.L, g.f, rd.dk, (long long *)nullptr, (long long *)nullptr, (unsigned long long *)nullptr,
                           (unsigned long long *)nullptr);
        GNS_HIP(hipGetLastError());
        GNS_TRY(rd.copy_out(keys, rd.dk, m * h->K, s));
    }
    if (start_ns) GNS_TRY(rd.copy_out(start_ns, g.f.start, m * 8, s));
    if (end_ns) GNS_TRY(rd.copy_out(end_ns, g.f.end, m * 8, s));
    if (pkts) GNS_TRY(rd.copy_out(pkts, g.f.pkts, m * 8, s));
    if (bytes) GNS_TRY(rd.copy_out(bytes, g.f.bytes, m * 8, s));
    if (written) GNS_TRY(rd.copy_out(written, g.written, m * 4, s));
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

int gns_ex_hist_trim(gns_ex_hist *h, int64_t before_ns, int fold, uint64_t out[4]) {
    if (!h) { set_error("null argument"); return GNS_E_ARG; }
    if (fold != 0 && fold != 1) { set_error("history trim: fold %d (0: drop, 1: fold)", fold); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    const HistPlan::Trim tp = h->plan.trim_plan(before_ns, fold != 0);
    if (out) { out[0] = out[1] = out[2] = 0; out[3] = h->plan.rows; }
    if (tp.noop) return GNS_OK;
    GNS_TRY(set_device(h->device));
    hipStream_t s = h->stream;
    HistIndex &ix = h->ix;
    const uint64_t old_slots = ix.slots;
    ExHistTrim t{};
    t.rows = h->plan.rows; t.R = tp.R; t.fold = tp.fold ? 1 : 0; t.d = tp.d; t.s_last = (uint32_t)(tp.c - 1);
    const bool ranked = tp.fold && tp.R != 0;  // prefix rows may stay
    t.row0 = ranked ? 0 : tp.R;
    GNS_TRY(ix.reserve_mark(old_slots));
    if (ranked) {  // flag and rank the prefix: V1 / V2 as of the last expired snapshot
        ExSelAsOf sel;
        ExTable T;
        sel.written = h->log.written; sel.superseded = h->log.superseded; sel.s = t.s_last;
        T = ExTable{h->log.L, h->log.f, tp.R};
        GNS_TRY(exh_rank(h, T, sel, &t.nb, &t.nbase));
    }
    const uint64_t kept = t.nbase + (t.rows - t.R);
    // everything new is built beside the history, which stays as it is until the end
    ExHistLog g;
    uint32_t *newrow = nullptr, *nh = nullptr;
    uint64_t forgot = 0;
    GNS_TRY(exh_alloc_log(h, hist_row_capacity(0, kept), &g));
    auto run = [&]() -> int {
        if (ranked) GNS_TRY(dalloc_t(&newrow, tp.R));
        const uint64_t span = t.rows - t.row0;
        if (span) {
            hipLaunchKernelGGL(k_exh_trim_move, dim3((unsigned)((span + 255) / 256)), dim3(256), 0, s, h->log, t,
                               (const uint32_t *)h->scan, g, newrow);
            GNS_HIP(hipGetLastError());
        }
        const dim3 sgrid((unsigned)((old_slots + 255) / 256));
        uint32_t *hp = reinterpret_cast<uint32_t *>(h->rd.po.pin);
        GNS_HIP(hipMemsetAsync(ix.fresh, 0, 4, s));
        hipLaunchKernelGGL(k_exh_trim_marks, sgrid, dim3(256), 0, s, (const uint32_t *)h->head, old_slots, t,
                           (const uint32_t *)newrow, ix.mark, ix.fresh);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipMemcpyAsync(hp, ix.fresh, 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));
        forgot = *hp;
        const uint32_t *remap = nullptr;
        if (forgot) {  // the index rebuilt from the keys that keep a row, into a table of their number
            const uint64_t want = hist_index_slots(h->keys - forgot);
            GNS_TRY(dalloc_t(&nh, want));
            GNS_HIP(hipMemsetAsync(nh, 0xFF, want * 4, s));
            GNS_TRY(ix.shrink_beside(want, s));
            remap = ix.dsc.remap;
        } else {
            GNS_TRY(dalloc_t(&nh, old_slots));
        }
        hipLaunchKernelGGL(k_exh_trim_heads, sgrid, dim3(256), 0, s, (const uint32_t *)h->head, old_slots, t,
                           (const uint32_t *)newrow, remap, nh);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipStreamSynchronize(s));
        return GNS_OK;
    };
    const int rc = run();
    if (rc != GNS_OK) {
        (void)hipStreamSynchronize(s);
        ix.rollback();
        exh_free_log(g);
        dfree(newrow); dfree(nh);
        return rc;
    }
    dfree(newrow);
    // publish: the log, the index and its head words, then the plan
    exh_free_log(h->log);
    h->log = g;
    dfree(h->head);
    h->head = nh;
    ix.commit();
    h->keys -= forgot;
    h->rows_trimmed += t.R - t.nbase;
    h->plan = h->plan.trimmed(tp, t.nbase);
    if (out) { out[0] = tp.fold ? tp.c - 1 : tp.c; out[1] = t.R - t.nbase; out[2] = forgot; out[3] = h->plan.rows; }
    return GNS_OK;
}

int gns_ex_hist_times(gns_ex_hist *h, int64_t *ts, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t n = h->plan.ts.size(), m = std::min<uint64_t>(*n_io, n);
    *n_io = n;
    if (ts && m) memcpy(ts, h->plan.ts.data(), m * sizeof(int64_t));
    return GNS_OK;
}

int gns_ex_hist_stats(gns_ex_hist *h, uint64_t out[8]) {
    if (!h || !out) { set_error("null argument"); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->plan.ts.size(); out[1] = h->plan.rows; out[2] = h->keys; out[3] = h->log.cap;
    out[4] = h->ix.slots; out[5] = h->ix.n_index_grow; out[6] = h->n_log_grow; out[7] = h->rows_trimmed;
    return GNS_OK;
}

int gns_ex_hist_aggregate(gns_ex_hist *h, const int64_t *end_ns, const gns_ex_filter *f, uint32_t nf, gns_ex_summary *out) {
    return exh_aggregate(h, end_ns, ExFilters(f), nf, out);
}

int gns_ex_hist_aggregate_cidr(gns_ex_hist *h, const int64_t *end_ns, const gns_ex_cidr *f, uint32_t nf,
                               gns_ex_summary *out) {
    return exh_aggregate(h, end_ns, ExFilters(f), nf, out);
}

int gns_ex_hist_heavy_hitters(gns_ex_hist *h, const int64_t *end_ns, int metric, uint64_t threshold, uint64_t limit,
                              uint8_t *keys, uint64_t *values, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    if (metric != 0 && metric != 1) { set_error("metric %d (0: PacketCount, 1: ByteCount)", metric); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    ExSelAsOf sel;
    ExTable T;
    (void)exh_as_of(h, end_ns, &sel, &T);
    return ex_heavy_on(h->K, T, h->stream, h->rd, nullptr, metric, threshold, limit, keys, values, n_io, &sel);
}

int gns_ex_hist_snapshot(gns_ex_hist *h, const int64_t *end_ns, uint8_t *keys, int64_t *start_ns, int64_t *end_out_ns,
                         uint64_t *pkts, uint64_t *bytes, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    ExSelAsOf sel;
    ExTable T;
    (void)exh_as_of(h, end_ns, &sel, &T);
    const uint64_t cap = *n_io;
    if (T.rows == 0) { *n_io = 0; return GNS_OK; }
    // V1-V3 over the log: the live rows compacted in log order
    hipStream_t s = h->stream;
    const uint32_t nblk = (uint32_t)((T.rows + 255) / 256);
    uint32_t nb = 0;
    uint64_t live = 0;
    GNS_TRY(exh_rank(h, T, sel, &nb, &live));
    const uint32_t *cnt = h->scan;
    const uint64_t m = std::min<uint64_t>(cap, live);
    *n_io = live;
    if (m == 0 || !(keys || start_ns || end_out_ns || pkts || bytes)) return GNS_OK;
    if (live > h->scap) {
        exv_free_rows(h->SD, h->sf);
        h->scap = 0;
        const uint64_t c = 2 * live;
        int rc;
        if ((rc = dalloc_t(&h->SD.rec, c * h->SD.RW)) || (rc = dalloc_t(&h->sf.pkts, c)) || (rc = dalloc_t(&h->sf.bytes, c)) ||
            (rc = dalloc_t(&h->sf.start, c)) || (rc = dalloc_t(&h->sf.end, c))) {
            exv_free_rows(h->SD, h->sf);
            return rc;
        }
        h->scap = c;
    }
    hipLaunchKernelGGL(k_exhv_write, dim3(nblk), dim3(256), 0, s, T.D, T.rows, T.f, sel, nb, cnt, h->SD, h->sf, h->scap);
    GNS_HIP(hipGetLastError());
    ExRead &rd = h->rd;
    if (keys) {
        GNS_TRY(rd.buf(&rd.dk, rd.dk_n, m * h->K));
        hipLaunchKernelGGL(k_ex_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const uint32_t *)nullptr, m,
                           h->SD, h->sf, rd.dk, (long long *)nullptr, (long long *)nullptr,
                           (unsigned long long *)nullptr, (unsigned long long *)nullptr);
        GNS_HIP(hipGetLastError());
        GNS_TRY(rd.copy_out(keys, rd.dk, m * h->K, s));
    }
    if (start_ns) GNS_TRY(rd.copy_out(start_ns, h->sf.start, m * 8, s));
    if (end_out_ns) GNS_TRY(rd.copy_out(end_out_ns, h->sf.end, m * 8, s));
    if (pkts) GNS_TRY(rd.copy_out(pkts, h->sf.pkts, m * 8, s));
    if (bytes) GNS_TRY(rd.copy_out(bytes, h->sf.bytes, m * 8, s));
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

int gns_ex_merge(gns_ex *ex, const uint8_t *keys, const int64_t *start_ns, const int64_t *end_ns,
                 const uint64_t *pkts, const uint64_t *bytes, uint64_t n, gns_mem where) {
    if (!ex || (n && (!keys || !start_ns || !end_ns || !pkts || !bytes))) { set_error("null argument"); return GNS_E_ARG; }
    if (n == 0) return GNS_OK;
    if (where == GNS_MEM_DEVICE && (((uintptr_t)start_ns | (uintptr_t)end_ns | (uintptr_t)pkts | (uintptr_t)bytes) & 7u)) {
        set_error("merge: device row arrays not 8-byte aligned");
        return GNS_E_ARG;
    }
    GNS_TRY(set_device(ex->device));
    hipStream_t s = ex->stream;
    KeyResolveScratch sc;
    uint32_t *ids = nullptr;
    GNS_TRY(dalloc_t(&ids, std::min<uint64_t>(n, kResolvePiece)));
    auto run = [&]() -> int {
        for (uint64_t off = 0; off < n; off += kResolvePiece) {
            const uint64_t m = std::min<uint64_t>(kResolvePiece, n - off);
            const uint8_t *dk = keys + off * ex->K;
            const long long *ds = reinterpret_cast<const long long *>(start_ns) + off;
            const long long *de = reinterpret_cast<const long long *>(end_ns) + off;
            const unsigned long long *dp = reinterpret_cast<const unsigned long long *>(pkts) + off;
            const unsigned long long *db = reinterpret_cast<const unsigned long long *>(bytes) + off;
            if (where != GNS_MEM_DEVICE) {  // stage the piece on the device
                StageList l;
                stage_add(l, dk, (size_t)m * ex->K, &dk);
                stage_add(l, ds, m * 8, &ds);
                stage_add(l, de, m * 8, &de);
                stage_add(l, dp, m * 8, &dp);
                stage_add(l, db, m * 8, &db);
                GNS_TRY(ex->stage.copy(l, s));
            }
            GNS_TRY(ex_resolve_rows(ex, dk, ex->K, m, dp, ids, sc, nullptr));
            const unsigned long long base = ex->pkt + ex->merged;
            const dim3 grid((unsigned)((m + 255) / 256));
            hipLaunchKernelGGL(k_ex_merge_add, grid, dim3(256), 0, s, ids, m, dp, db, base, ex->f);
            hipLaunchKernelGGL(k_ex_merge_times, grid, dim3(256), 0, s, ids, m, ds, de, base, ex->f);
            GNS_HIP(hipGetLastError());
            ex->merged += m;
        }
        GNS_TRY(ex_hot_clear(ex));  // the next batch re-picks the designated flows
        GNS_HIP(hipStreamSynchronize(s));
        return GNS_OK;
    };
    const int rc = run();
    if (rc != GNS_OK) (void)hipStreamSynchronize(s);
    dfree(ids);
    sc.free_all();
    return rc;
}

namespace {

void exr_free(ExrRows &R) {
    dfree(R.keys); dfree(R.ids); dfree(R.cnt); dfree(R.pkts); dfree(R.bytes); dfree(R.first); dfree(R.last);
    dfree(R.start); dfree(R.end);
    R = ExrRows{};
}

// The projection plan from layout `from` onto layout `to`: *pl (px == nullptr) or *pp is filled.
// GNS_E_ARG names the first field of `to` that `from` lacks.
int exr_plans(const KeyPlanN &from, const KeyPlanN &to, const gns_prefix *px, const char *what, ExrPlan<false> *pl,
              ExrPlan<true> *pp) {
    pl->K = pp->K = to.K;
    pl->KW = pp->KW = (to.K + 3) / 4;
    int miss;
    if (px) {
        RollRow row;
        memset(pp->ipoff, 0xFF, sizeof(pp->ipoff));
        miss = roll_tables(from.src, from.K, to.src, to.K, px, false, &row, pp->ipoff);
        memcpy(pp->t, &row, sizeof(pp->t));
    } else {
        miss = roll_gather(from.src, from.K, to.src, to.K, pl->t);
    }
    if (miss >= 0) {
        set_error("%s: key field %s is not part of the source's layout", what, tuple_field_name(to.src[miss]));
        return GNS_E_ARG;
    }
    return GNS_OK;
}

// gns_ex_rollup (px == nullptr) and gns_ex_rollup_prefix behind their argument checks
static int exr_rollup(gns_ex *dst, gns_ex *src, const gns_prefix *px, uint64_t out[2]) {
    if (dst == src) { set_error("rollup: dst and src are the same handle"); return GNS_E_ARG; }
    if (dst->device != src->device) {
        set_error("rollup: dst is on device %d, src on device %d", dst->device, src->device);
        return GNS_E_ARG;
    }
    ExrPlan<false> pl{};  // the one the call takes is filled
    ExrPlan<true> pp{};
    GNS_TRY(exr_plans(src->kp, dst->kp, px, "rollup", &pl, &pp));
    GNS_TRY(set_device(dst->device));
    const uint64_t piece = std::min<uint64_t>(test_piece("GNS_EX_ROLLUP_PIECE", kResolvePiece), src->slots);
    if (out) out[0] = out[1] = 0;
    hipStream_t s = dst->stream;
    ExrRows R{};
    KeyResolveScratch sc;
    uint64_t projected = 0, added = 0;
    bool wrote = false;
    auto run = [&]() -> int {
        int rc;
        if ((rc = dalloc_t(&R.keys, piece * pl.KW)) || (rc = dalloc_t(&R.ids, piece)) || (rc = dalloc_t(&R.cnt, 4)) ||
            (rc = dalloc_t(&R.pkts, piece)) || (rc = dalloc_t(&R.bytes, piece)) || (rc = dalloc_t(&R.first, piece)) ||
            (rc = dalloc_t(&R.last, piece)) || (rc = dalloc_t(&R.start, piece)) || (rc = dalloc_t(&R.end, piece)))
            return rc;
        GNS_TRY(stream_wait_now(s, src->stream, "rollup"));  // after src's pending batches
        const unsigned long long B = dst->pkt + dst->merged;  // source positions lie behind dst's stream end
        for (uint64_t s0 = 0; s0 < src->slots; s0 += piece) {
            const uint64_t s1 = std::min<uint64_t>(s0 + piece, src->slots);
            GNS_HIP(hipMemsetAsync(R.cnt, 0, 4, s));
            const dim3 grid((unsigned)((s1 - s0 + 255) / 256));
            if (px) hipLaunchKernelGGL(k_exr_project<true>, grid, dim3(256), 0, s, src->D, src->f, s0, s1, pp, R);
            else hipLaunchKernelGGL(k_exr_project<false>, grid, dim3(256), 0, s, src->D, src->f, s0, s1, pl, R);
            GNS_HIP(hipGetLastError());
            GNS_HIP(hipMemcpyAsync(dst->h_pin, R.cnt, 4, hipMemcpyDeviceToHost, s));
            GNS_HIP(hipStreamSynchronize(s));
            const uint64_t m = std::min<uint64_t>(dst->h_pin[0], s1 - s0);
            if (m == 0) continue;
            GNS_TRY(ex_resolve_rows(dst, reinterpret_cast<const uint8_t *>(R.keys), 4 * pl.KW, m, R.pkts, R.ids, sc, &added));
            wrote = true;
            hipLaunchKernelGGL(k_exr_add, dim3((unsigned)std::min<uint64_t>((m + 255) / 256, 1024)), dim3(256), 0, s, R, m,
                               B, dst->f);
            hipLaunchKernelGGL(k_exr_times, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, R, m, B, dst->f);
            GNS_HIP(hipGetLastError());
            projected += m;
        }
        return GNS_OK;
    };
    int rc = run();
    if (rc == GNS_OK || wrote) {
        // the positions handed out are spent, whatever happened after the first piece
        dst->merged += src->pkt + src->merged;
        const int rc2 = ex_hot_clear(dst);  // the next batch re-picks the designated flows
        if (rc == GNS_OK) rc = rc2;
    }
    if (hipStreamSynchronize(s) != hipSuccess && rc == GNS_OK) { set_error("rollup: stream synchronize failed"); rc = GNS_E_HIP; }
    exr_free(R);
    sc.free_all();
    if (rc == GNS_OK && out) { out[0] = projected; out[1] = added; }
    return rc;
}

}  // namespace

int gns_ex_rollup(gns_ex *dst, gns_ex *src, uint64_t out[2]) {
    if (!dst || !src) { set_error("null argument"); return GNS_E_ARG; }
    return exr_rollup(dst, src, nullptr, out);
}

int gns_ex_rollup_prefix(gns_ex *dst, gns_ex *src, const gns_prefix *px, uint64_t out[2]) {
    if (!dst || !src) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(px_check_prefix(px, "rollup"));
    return exr_rollup(dst, src, px, out);
}

namespace {
// gns_ex_hist_rollup (window == false: the rows live as of end_ns) and gns_ex_hist_rollup_between
// (the plus and minus rows of the window (start_ns, end_ns]): one body, two H1 selections
int exh_rollup(gns_ex *dst, gns_ex_hist *h, bool window, const int64_t *start_ns, const int64_t *end_ns,
               const gns_prefix *px, uint64_t out[2]) {
    if (!dst || !h) { set_error("null argument"); return GNS_E_ARG; }
    if (window && start_ns && end_ns && *start_ns > *end_ns) {
        set_error("history rollup: the window starts at %lld, after its end %lld", (long long)*start_ns, (long long)*end_ns);
        return GNS_E_ARG;
    }
    if (px) GNS_TRY(px_check_prefix(px, "history rollup"));
    if (dst->device != h->device) {
        set_error("history rollup: dst is on device %d, the history on device %d", dst->device, h->device);
        return GNS_E_ARG;
    }
    ExrPlan<false> pl{};
    ExrPlan<true> pp{};
    GNS_TRY(exr_plans(h->kp, dst->kp, px, "history rollup", &pl, &pp));
    GNS_TRY(set_device(dst->device));
    if (out) out[0] = out[1] = 0;
    // a reader call on the history: held until dst's stream has drained, so no trim frees the
    // log under the kernels and an append waits
    std::lock_guard<std::mutex> lk(h->mu);
    ExSelAsOf sel;
    ExSelBetween bsel{};
    ExTable T;
    if (window) {
        const HistPlan::Between b = h->plan.between(start_ns, end_ns);
        bsel = ExSelBetween{h->log.superseded, (uint32_t)(b.s0 + 1), (uint32_t)b.s1, b.minus_end};
        T = ExTable{h->log.L, h->log.f, b.empty ? 0 : b.scan_end};  // (bad: checked above)
    } else {
        (void)exh_as_of(h, end_ns, &sel, &T);
    }
    const uint64_t rows = T.rows;
    if (rows == 0) return GNS_OK;  // no snapshot at or before the time (or none with rows; no snapshot in the window): an empty source
    const uint64_t piece = std::min<uint64_t>(test_piece("GNS_EX_ROLLUP_PIECE", kResolvePiece), rows);
    hipStream_t s = dst->stream;
    ExrRows R{};
    KeyResolveScratch sc;
    uint64_t projected = 0, added = 0;
    bool wrote = false;
    auto run = [&]() -> int {
        int rc;
        if ((rc = dalloc_t(&R.keys, piece * pl.KW)) || (rc = dalloc_t(&R.ids, piece)) || (rc = dalloc_t(&R.cnt, 4)) ||
            (rc = dalloc_t(&R.pkts, piece)) || (rc = dalloc_t(&R.bytes, piece)) || (rc = dalloc_t(&R.first, piece)) ||
            (rc = dalloc_t(&R.start, piece)) || (rc = dalloc_t(&R.end, piece)))
            return rc;
        GNS_TRY(stream_wait_now(s, h->stream, "history rollup"));  // after the history's pending work
        const unsigned long long B = dst->pkt + dst->merged;  // log row r stands at position B + r
        for (uint64_t r0 = 0; r0 < rows; r0 += piece) {
            const uint64_t r1 = std::min<uint64_t>(r0 + piece, rows);
            GNS_HIP(hipMemsetAsync(R.cnt, 0, 4, s));
            const dim3 grid((unsigned)((r1 - r0 + 255) / 256));
            if (window && px) hipLaunchKernelGGL((k_exh_project<true, ExSelBetween>), grid, dim3(256), 0, s, T.D, T.f, bsel, r0, r1, pp, R);
            else if (window) hipLaunchKernelGGL((k_exh_project<false, ExSelBetween>), grid, dim3(256), 0, s, T.D, T.f, bsel, r0, r1, pl, R);
            else if (px) hipLaunchKernelGGL(k_exh_project<true>, grid, dim3(256), 0, s, T.D, T.f, sel, r0, r1, pp, R);
            else hipLaunchKernelGGL(k_exh_project<false>, grid, dim3(256), 0, s, T.D, T.f, sel, r0, r1, pl, R);
            GNS_HIP(hipGetLastError());
            GNS_HIP(hipMemcpyAsync(dst->h_pin, R.cnt, 4, hipMemcpyDeviceToHost, s));
            GNS_HIP(hipStreamSynchronize(s));
            const uint64_t m = std::min<uint64_t>(dst->h_pin[0], r1 - r0);
            if (m == 0) continue;
            GNS_TRY(ex_resolve_rows(dst, reinterpret_cast<const uint8_t *>(R.keys), 4 * pl.KW, m, R.pkts, R.ids, sc, &added,
                                    window));
            wrote = true;
            hipLaunchKernelGGL(k_exh_seed, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const uint32_t *)R.ids, m,
                               dst->f);
            hipLaunchKernelGGL(k_exh_add, dim3((unsigned)std::min<uint64_t>((m + 255) / 256, 1024)), dim3(256), 0, s, R, m,
                               B, dst->f);
            GNS_HIP(hipGetLastError());
            projected += m;
        }
        return GNS_OK;
    };
    int rc = run();
    if (rc == GNS_OK || wrote) {
        // the positions handed out are spent, whatever happened after the first piece
        dst->merged += rows;
        const int rc2 = ex_hot_clear(dst);  // the next batch re-picks the designated flows
        if (rc == GNS_OK) rc = rc2;
    }
    if (hipStreamSynchronize(s) != hipSuccess && rc == GNS_OK) {
        set_error("history rollup: stream synchronize failed");
        rc = GNS_E_HIP;
    }
    exr_free(R);
    sc.free_all();
    if (rc == GNS_OK && out) { out[0] = projected; out[1] = added; }
    return rc;
}
}  // namespace

int gns_ex_hist_rollup(gns_ex *dst, gns_ex_hist *h, const int64_t *end_ns, const gns_prefix *px, uint64_t out[2]) {
    return exh_rollup(dst, h, false, nullptr, end_ns, px, out);
}

int gns_ex_hist_rollup_between(gns_ex *dst, gns_ex_hist *h, const int64_t *start_ns, const int64_t *end_ns,
                               const gns_prefix *px, uint64_t out[2]) {
    return exh_rollup(dst, h, true, start_ns, end_ns, px, out);
}

int gns_ex_reset(gns_ex *ex) {
    if (!ex) return GNS_E_ARG;
    GNS_TRY(set_device(ex->device));
    GNS_TRY(ex_clear(ex));
    GNS_HIP(hipStreamSynchronize(ex->stream));
    return GNS_OK;
}

int gns_ex_counters(gns_ex *ex, uint64_t out[8]) {
    if (!ex || !out) return GNS_E_ARG;
    GNS_TRY(set_device(ex->device));
    GNS_HIP(hipStreamSynchronize(ex->stream));
    unsigned long long h[8];
    GNS_HIP(hipMemcpy(h, ex->stats, sizeof(h), hipMemcpyDeviceToHost));
    uint64_t nf = 0;
    GNS_TRY(gns_ex_snapshot(ex, nullptr, nullptr, nullptr, nullptr, nullptr, &nf));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = h[3];
    out[4] = nf; out[5] = ex->pkt; out[6] = ex->batches; out[7] = 0;
    return GNS_OK;
}

int gns_ex_dict_stats(gns_ex *ex, uint64_t out[8]) {
    if (!ex || !out) return GNS_E_ARG;
    out[0] = ex->n_grow; out[1] = 0; out[2] = ex->slots; out[3] = ex->claimed;
    out[4] = (uint64_t)(ex->grow_ms * 1000.0); out[5] = ex->n_retry;
    out[6] = ex->slots; out[7] = ex->n_grow;
    return GNS_OK;
}

int gns_ex_set_timing(gns_ex *ex, int on) {
    if (!ex) return GNS_E_ARG;
    set_timing_arg(ex->timer, on);
    return GNS_OK;
}

int gns_ex_stage_times(gns_ex *ex, double ms[8], uint64_t launches[8], int reset) {
    if (!ex) return GNS_E_ARG;
    GNS_TRY(set_device(ex->device));
    ex->timer.report(ms, launches, reset);
    return GNS_OK;
}

}  // extern "C"
