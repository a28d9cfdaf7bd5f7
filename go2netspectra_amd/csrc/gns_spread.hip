// gns_spread.hip -- exact distinct-element (spread) aggregator: the device
// ground truth of SuperSpread (ss_test.go:49-66,86-136 keep a
// map[flow]map[elem]bool; spread(flow) = len of the inner map).
//
// Semantics: spread(flow) = number of distinct element keys inserted together
// with that flow key since create / the last reset.  Exact: pairs are compared by
// their bytes, a pair is counted once however its duplicates are spread over
// lanes, waves, workgroups, device batches and calls, and the result does not
// depend on packet order.
//
// State:
//   pair table  open addressing, keyed by the pair's own bytes flow ‖ elem
//               (<= 74): records {tag, key words} of 16 or 32 words, the tag and
//               epoch protocol of the flow dictionary (gns_keys.cuh).  Flow ids
//               are not part of the key, so a growing flow table never forces a
//               rehash of the pairs.
//   flow table  a DictDev over the flow bytes; spread[slot] is the flow's count.
//
// One device batch:
//   E1 k_exs_pass<FIRST>   parse, flow and pair key words, probe the pair table.
//        committed equal record -> duplicate, done (one line read, no write)
//        claimed an empty slot  -> NEW pair: find-or-claim the flow, spread += 1
//                                  (folded per workgroup in LDS: a hot flow costs
//                                  one global add per workgroup)
//        slot claimed in this launch (its bytes are not visible yet) -> parked
//   E2 k_exs_pass<!FIRST>  the parked packets re-probe from where they stopped,
//        under a new epoch (the kernel boundary committed the claims); a NEW pair
//        whose flow slot was pending is parked as "count only".  Repeats until
//        no packet is parked; the first repeat is queued blind, then one host
//        read per round (rarely more than one).
// The NEW outcome is unique per pair (one CAS wins the empty slot), and only it
// counts: that is the whole exactness argument.
//
// Growth: decided BEFORE a batch from host-known bounds.  A batch of m packets
// claims at most m pair slots and m flow slots, so both tables are grown (pair
// table: rehash of its own records; flow table: dict_rebuild with every flow
// live, spread[] permuted by its remap) until claimed + m <= 3/4 of the slots.
// No batch can overflow a table, so none is aborted or re-run and nothing can be
// counted twice (DESIGN.md §4e states why this replaces the abort-and-retry of
// the sketches).
//
// State interface (gns_pairs_*, DESIGN.md §4e "Pair set export and union"): the
// pair set is the state.  k_exs_export compacts the live records -- all, or those
// whose tag (the claim epoch) is newer than a cursor -- into dense flow / element
// rows; a merge feeds such rows through k_exs_pass in a mode that counts no
// traffic; merge_from does both between two handles on the device.  Cursors are
// generation << 32 | epoch; a reset and the epoch's wrap (k_exs_retag) start a
// new generation.
//
// Spread roll-up (gns_spread_rollup, DESIGN.md §4e "Spread roll-up"): the distinct
// (flow, element) pairs of a stream are the projection of its distinct flow keys
// whenever both layouts are made of fields of an exact aggregator's key.
// k_spr_project turns pieces of such an aggregator's table into staged pair rows --
// IP fields from the aggregator's To16 form back to EncodeFlow form -- and the rows
// enter through the merge mode of k_exs_pass.
#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

#include "gns_common.hpp"
#include "gns_ctl.cuh"
#include "gns_exsrc.hpp"
#include "gns_hh.hpp"

namespace gns {

constexpr int kExsThreads = 256;
constexpr uint32_t kExsChunk = 4096;   // packets per workgroup; a parked entry keeps 12 bits of packet index
constexpr uint32_t kExsFold = 512;     // LDS (flow id, new pairs) entries per workgroup
constexpr uint64_t kExsMaxPairSlots = 1ull << 31;

struct PairDev {
    uint32_t *rec;   // slots * RW words: tag (0 empty, else claim epoch), key words
    uint32_t mask;   // slots - 1
    uint32_t RW;     // 16 or 32 (one or two 64-byte lines, never straddling)
    uint32_t seed;
    uint32_t K;      // pair key bytes
};

enum { PAIR_DUP = 0, PAIR_NEW = 1, PAIR_PENDING = 2, PAIR_FULL = 3 };

// LW uint4 loads cover the tag and the key words the kernel's word count can hold
template <int LW>
__device__ __forceinline__ void pair_load(const PairDev &P, uint32_t slot, uint32_t (&r)[4 * LW]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(P.rec + (size_t)slot * P.RW);
#pragma unroll
    for (int i = 0; i < LW; i++) {
        const uint4 v = (4u * i < P.RW) ? q[i] : make_uint4(0, 0, 0, 0);
        r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
}

// dict_find_or_claim (gns_keys.cuh) for pair keys of NW words.  Every probe
// sequence ends: the host keeps claimed < slots, so an empty slot exists.
template <int NW>
__device__ __forceinline__ int pair_find_or_claim(const PairDev &P, const uint32_t (&kw)[NW], uint32_t slot,
                                                  uint32_t epoch, uint32_t *out) {
    constexpr int LW = NW <= 8 ? 3 : 5;  // 8 key words + tag; 19 key words (74 bytes) + tag
    const uint32_t nkw = (P.K + 3) >> 2;
    for (uint32_t probe = 0; probe <= P.mask; probe++) {
        uint32_t r[4 * LW];
        pair_load<LW>(P, slot, r);
        uint32_t tag = r[0];
        if (tag == 0) {
            uint32_t *tp = P.rec + (size_t)slot * P.RW;
            const uint32_t old = atomicCAS(tp, 0u, epoch);
            if (old == 0) {
#pragma unroll
                for (int i = 0; i < NW; i++)
                    if ((uint32_t)i < nkw) tp[1 + i] = kw[i];
                *out = slot;
                return PAIR_NEW;
            }
            tag = old;
            if (tag != epoch) pair_load<LW>(P, slot, r);  // committed earlier: need its key words
        }
        if (tag == epoch) { *out = slot; return PAIR_PENDING; }
        bool eq = true;
#pragma unroll
        for (int i = 0; i < NW; i++)
            if ((uint32_t)i < nkw && 1 + i < 4 * LW) eq = eq && (r[1 + i] == kw[i]);
        if (eq) { *out = slot; return PAIR_DUP; }
        slot = (slot + 1u) & P.mask;
    }
    return PAIR_FULL;
}

struct ExsArgs {
    InputDesc in;
    uint64_t n;
    KeyPlanN kpf, kpm;
    uint32_t Kf, Km;
    PairDev P;
    DictDev F;
    uint32_t epoch;
    uint32_t *spread;
    uint32_t *nclaim;            // [0] flow slots, [1] pair slots claimed since the last reset
    const uint64_t *pend_in;     // parked: stage << 63 | (packet - chunk start) << 32 | slot to resume at
    const uint32_t *cnt_in;      // [chunk]
    uint64_t *pend_out;
    uint32_t *cnt_out, *total_out;
    unsigned long long *stats;   // 0 inserted, 1 dropped, 2 unsupported, 3 probe overflow (cannot), 4 new pairs
    uint32_t merge;              // the rows are a pair set being united (gns_pairs_merge), not traffic: stats[0] stays
};

// flow key (kwf) and pair key flow ‖ elem (kwm) of packet p: the bytes SuperSpread
// hashes (EncodeFlow, task.go:265-300; super_spread.go:183-190)
template <int KIND, int MF, int MM, int NW>
__device__ __forceinline__ int exs_keys(const ExsArgs &a, const uint8_t *s_srcf, const uint8_t *s_srcm, uint64_t p,
                                        uint32_t (&kwf)[GNS_KWMAX], uint32_t (&kwm)[NW]) {
    if constexpr (KIND == IN_KEYS) {
        const uint8_t *f = a.in.keys + p * a.in.stride;
        const uint8_t *e = a.in.keys2 + p * a.in.stride2;
        load_key_bytes<GNS_KWMAX>(f, a.Kf, false, kwf);
#pragma unroll
        for (int i = 0; i < NW; i++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t j = 4 * i + b;
                uint32_t byte = 0;
                if (j < a.Kf) byte = f[j];
                else if (j < a.Km) byte = e[j - a.Kf];
                v |= byte << (8 * b);
            }
            kwm[i] = v;
        }
        return PARSE_OK;
    } else {
        uint32_t tw[10];
        const int st = load_tuple<KIND>(a.in, p, tw);
        if (st != PARSE_OK) return st;
        make_key_m<MF, GNS_KWMAX>(a.Kf, s_srcf, tw, kwf);
        make_key_m<MM, NW>(a.Km, s_srcm, tw, kwm);
        return PARSE_OK;
    }
}

// One pass over a chunk of kExsChunk packets per workgroup: FIRST = every packet
// of the chunk from its hash slot, else the chunk's parked packets.
template <int KIND, int MF, int MM, int NW, bool FIRST>
__global__ __launch_bounds__(kExsThreads) void k_exs_pass(ExsArgs a) {
    __shared__ uint8_t s_srcf[80], s_srcm[80];
    __shared__ uint32_t s_fid[kExsFold], s_fcnt[kExsFold];
    __shared__ uint32_t s_cnt, s_new, s_fclaim, s_full, s_ok, s_drop, s_unsup;
    const uint32_t tid = threadIdx.x, ch = blockIdx.x;
    for (uint32_t j = tid; j < 80; j += kExsThreads) { s_srcf[j] = a.kpf.src[j]; s_srcm[j] = a.kpm.src[j]; }
    for (uint32_t j = tid; j < kExsFold; j += kExsThreads) { s_fid[j] = GNS_ID_NONE; s_fcnt[j] = 0; }
    if (tid == 0) { s_cnt = 0; s_new = 0; s_fclaim = 0; s_full = 0; s_ok = 0; s_drop = 0; s_unsup = 0; }
    __syncthreads();
    const uint64_t beg = (uint64_t)ch * kExsChunk;
    const uint32_t cnt = FIRST ? (uint32_t)min((uint64_t)kExsChunk, a.n - beg) : a.cnt_in[ch];
    for (uint32_t i = tid; i < cnt; i += kExsThreads) {
        uint32_t rel = i, slot = 0, stage = 0;
        if (!FIRST) {
            const uint64_t v = a.pend_in[beg + i];
            stage = (uint32_t)(v >> 63);
            rel = (uint32_t)(v >> 32) & (kExsChunk - 1);
            slot = (uint32_t)v;
        }
        uint32_t kwf[GNS_KWMAX], kwm[NW];
        const int st = exs_keys<KIND, MF, MM, NW>(a, s_srcf, s_srcm, beg + rel, kwf, kwm);
        if (st != PARSE_OK) {  // only in the first pass: a parked packet parsed OK
            if (FIRST) atomicAdd(st == PARSE_DROP ? &s_drop : &s_unsup, 1u);
            continue;
        }
        if (FIRST) {
            atomicAdd(&s_ok, 1u);
            slot = mm3_n<NW>(kwm, a.Km, a.P.seed) & a.P.mask;
        }
        if (stage == 0) {
            uint32_t at;
            const int res = pair_find_or_claim<NW>(a.P, kwm, slot, a.epoch, &at);
            if (res == PAIR_DUP) continue;
            if (res == PAIR_PENDING) {
                a.pend_out[beg + atomicAdd(&s_cnt, 1u)] = (uint64_t)rel << 32 | at;
                continue;
            }
            if (res == PAIR_FULL) { atomicAdd(&s_full, 1u); continue; }
            atomicAdd(&s_new, 1u);
            slot = mm3_n<GNS_KWMAX>(kwf, a.Kf, a.F.seed) & a.F.mask;
        }
        // the packet holds a NEW pair: its flow's count goes up by one, exactly once
        uint32_t id;
        const int fr = dict_find_or_claim(a.F, kwf, slot, a.epoch, &id);
        if (fr == DICT_CLAIMED) atomicAdd(&s_fclaim, 1u);
        if (fr == DICT_FOUND || fr == DICT_CLAIMED) {
            const uint32_t h = (id * 0x9E3779B1u) >> 23;  // kExsFold = 2^9 entries
            const uint32_t old = atomicCAS(&s_fid[h], GNS_ID_NONE, id);
            if (old == GNS_ID_NONE || old == id) atomicAdd(&s_fcnt[h], 1u);
            else atomicAdd(&a.spread[id], 1u);
        } else if (fr == DICT_PENDING) {
            a.pend_out[beg + atomicAdd(&s_cnt, 1u)] = 1ull << 63 | (uint64_t)rel << 32 | id;
        } else {
            atomicAdd(&s_full, 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < kExsFold; j += kExsThreads)
        if (s_fcnt[j]) atomicAdd(&a.spread[s_fid[j]], s_fcnt[j]);
    if (tid == 0) {
        a.cnt_out[ch] = s_cnt;
        if (s_cnt) atomicAdd(a.total_out, s_cnt);
        if (s_fclaim) atomicAdd(&a.nclaim[0], s_fclaim);
        if (s_new) {
            atomicAdd(&a.nclaim[1], s_new);
            atomicAdd(&a.stats[4], (unsigned long long)s_new);
        }
        if (s_full) atomicAdd(&a.stats[3], (unsigned long long)s_full);
        if (s_ok && !a.merge) atomicAdd(&a.stats[0], (unsigned long long)s_ok);
        if (s_drop) atomicAdd(&a.stats[1], (unsigned long long)s_drop);
        if (s_unsup) atomicAdd(&a.stats[2], (unsigned long long)s_unsup);
    }
}

// pair-table growth: every record of the old table into the (zeroed) new one;
// keys are distinct, so the first empty slot from the home slot is its place
template <int NW>
__global__ __launch_bounds__(256) void k_exs_rehash(PairDev O, uint64_t old_slots, PairDev N, uint32_t *fail) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= old_slots) return;
    const uint32_t *r = O.rec + (size_t)s * O.RW;
    const uint32_t tag = r[0];
    if (tag == 0) return;
    const uint32_t nkw = (O.K + 3) >> 2;
    uint32_t kw[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) kw[i] = (uint32_t)i < nkw ? r[1 + i] : 0u;
    uint32_t slot = mm3_n<NW>(kw, N.K, N.seed) & N.mask;
    for (uint32_t probe = 0; probe <= N.mask; probe++) {
        uint32_t *tp = N.rec + (size_t)slot * N.RW;
        if (atomicCAS(tp, 0u, tag) == 0u) {
#pragma unroll
            for (int i = 0; i < NW; i++)
                if ((uint32_t)i < nkw) tp[1 + i] = kw[i];
            return;
        }
        slot = (slot + 1u) & N.mask;
    }
    atomicAdd(fail, 1u);
}

// one exported row: the record's key words split at Kf into flows[j * Kf] and elems[j * (K - Kf)].
// WORDS: both key sizes are multiples of 4 and both buffers word-aligned.
template <int NW, int LW, bool WORDS>
__device__ __forceinline__ void pair_store_row(const PairDev &P, const uint32_t (&r)[4 * LW], uint32_t Kf, uint64_t j,
                                               uint8_t *flows, uint8_t *elems) {
    const uint32_t Ke = P.K - Kf;
    if constexpr (WORDS) {
        uint32_t *fo = reinterpret_cast<uint32_t *>(flows + j * Kf);
        uint32_t *eo = reinterpret_cast<uint32_t *>(elems + j * Ke);
        const uint32_t fw = Kf >> 2, nw = P.K >> 2;
#pragma unroll
        for (int i = 0; i < NW; i++) {
            if (1 + i >= 4 * LW) continue;
            if ((uint32_t)i < fw) fo[i] = r[1 + i];
            else if ((uint32_t)i < nw) eo[i - fw] = r[1 + i];
        }
    } else {
        uint8_t *fo = flows + j * Kf, *eo = elems + j * Ke;
#pragma unroll
        for (int i = 0; i < NW; i++) {
            if (1 + i >= 4 * LW) continue;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t k = 4 * i + b;
                const uint8_t v = (uint8_t)(r[1 + i] >> (8 * b));
                if (k < Kf) fo[k] = v;
                else if (k < P.K) eo[k - Kf] = v;
            }
        }
    }
}

// Pair set export: the live records of slots [beg, end) -- tag non-zero and newer
// than `since` (0: every record) -- as dense rows.  A workgroup takes kExsExportIt
// runs of 256 slots, one lane per slot and run; a ballot per wave and run ranks the
// live lanes, and ONE atomic per workgroup reserves its rows (a table of 2^27 slots
// is 2^17 adds on the count word, not 2^21).  Rows at or past cap are counted and
// not written.  The records are committed (an export runs between batches), so
// their key words are visible.
constexpr int kExsExportIt = 4;
template <int NW, bool WORDS>
__global__ __launch_bounds__(256) void k_exs_export(PairDev P, uint64_t beg, uint64_t end, uint32_t since, uint32_t Kf,
                                                    uint8_t *flows, uint8_t *elems, uint64_t cap, uint32_t *count) {
    constexpr int LW = NW <= 8 ? 3 : 5, IT = kExsExportIt;
    __shared__ uint32_t s_cnt[IT * 4], s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t s0 = beg + (uint64_t)blockIdx.x * (256 * IT) + tid;
    uint32_t r[IT][4 * LW];
    uint64_t m[IT];
    bool live[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const uint64_t s = s0 + (uint64_t)it * 256;
        live[it] = false;
        if (s < end) {
            pair_load<LW>(P, (uint32_t)s, r[it]);
            live[it] = r[it][0] > since;
        }
        m[it] = __ballot(live[it]);
        if (lane == 0) s_cnt[it * 4 + wave] = (uint32_t)__popcll(m[it]);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int k = 0; k < IT * 4; k++) tot += s_cnt[k];
        s_base = tot ? atomicAdd(count, tot) : 0u;
    }
    __syncthreads();
    uint64_t run = s_base;  // rows of the workgroup's (run, wave) cells before this lane's
#pragma unroll
    for (int it = 0; it < IT; it++) {
        uint64_t j = run + (uint32_t)__popcll(m[it] & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t c = s_cnt[it * 4 + w];
            if ((uint32_t)w < wave) j += c;
            run += c;
        }
        if (live[it] && j < cap) pair_store_row<NW, LW, WORDS>(P, r[it], Kf, j, flows, elems);
    }
}

// Spread roll-up, projection: the flows of slots [beg, end) of an exact aggregator's
// table -- k_exr_project's occupancy rule (tag and pkts nonzero), first >= since -- as
// pair rows appended behind the *count rows already staged.  Ranking and reservation
// are k_exs_export's: kSprIt runs of 256 slots per workgroup, a ballot per wave and
// run, ONE atomic per workgroup.  A selected lane copies its key words into its own
// LDS column (no other lane touches it: no barrier), rewrites the IP fields the
// layouts read from To16 to EncodeFlow form there, and gathers the flow row and the
// element row byte by byte through the plan (copied into LDS once per workgroup),
// each row into words of its own, so a split inside a word costs nothing.
// Rows at or past cap are counted and not written.
//
// PX (gns_spread_rollup_prefix): the IP fields of the flow row and of the element row masked
// to a prefix, each row by tables of its own -- the prime uses read one field twice
// ("distinct source hosts per source /24": flow = SrcIP under /24, element = SrcIP whole).
// The masks are defined on the To16 bytes, so a lane takes its IPv4 flag per IP field BEFORE
// spr_encode_ip rewrites the column; after the rewrite an IPv4 address sits in bytes 0..3 of
// the field, and m4 is laid out for that (EncodeFlow) form.
//
// The plan: per row (flow, then element) the tables proj_word<PX> reads -- the gather g alone,
// or a whole RollRow.  They sit in LDS (one broadcast read per byte): as scalars the 74 plan
// bytes of the widest layout, live across the unrolled runs, spilled 270 SGPRs.
// The IP fields either row reads: PX keeps them per field, as roll_tables gives them; the plain
// plan keeps a count and a list (iplist), which the generated code depends on (below).
template <bool PX>
struct SprPlan {
    static constexpr int kRow = 40;  // bytes of a row's tables
    uint32_t Kf, Ke;         // the destination's flow / element key bytes
    uint32_t nip;            // IP fields of the source key that the rows read
    uint8_t iplist[4];       // their byte offsets in the source key, in any order
    union {                  // as words for the copy into LDS
        uint8_t t[2][kRow];
        uint32_t w[2 * kRow / 4];
    };
};
template <>
struct SprPlan<true> {
    static constexpr int kRow = (int)sizeof(RollRow);
    uint32_t Kf, Ke;
    uint8_t ipoff[4];        // byte offset of SrcIP / DstIP in the source key; 0xFF: not read by either row
    union {
        uint8_t t[2][kRow];
        uint32_t w[2 * kRow / 4];
    };
};
constexpr int kSprIt = 4;

template <bool PX, bool WORDS>
__global__ __launch_bounds__(256) void k_spr_project(DictDev S, const unsigned long long *pkts,
                                                     const unsigned long long *first, uint64_t beg, uint64_t end,
                                                     unsigned long long since, SprPlan<PX> pl, uint8_t *flows,
                                                     uint8_t *elems, uint64_t cap, uint32_t *count) {
    constexpr int IT = kSprIt, NW = 2 * SprPlan<PX>::kRow / 4;
    __shared__ uint32_t s_k[GNS_KWMAX][256];
    __shared__ uint32_t s_cnt[IT * 4], s_base;
    __shared__ uint32_t s_pw[NW];  // the flow row's tables, then the element row's
    const uint8_t *s_t = reinterpret_cast<const uint8_t *>(s_pw);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t s0 = beg + (uint64_t)blockIdx.x * (256 * IT) + tid;
    if (tid < NW) s_pw[tid] = pl.w[tid];
    uint64_t m[IT];
    bool live[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) {
        const uint64_t s = s0 + (uint64_t)it * 256;
        live[it] = s < end && S.rec[s * S.RW] != 0u && pkts[s] != 0ull && first[s] >= since;
        m[it] = __ballot(live[it]);
        if (lane == 0) s_cnt[it * 4 + wave] = (uint32_t)__popcll(m[it]);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int k = 0; k < IT * 4; k++) tot += s_cnt[k];
        s_base = tot ? atomicAdd(count, tot) : 0u;
    }
    __syncthreads();
    uint64_t run = s_base;  // rows of the workgroup's (run, wave) cells before this lane's
#pragma unroll
    for (int it = 0; it < IT; it++) {
        uint64_t j = run + (uint32_t)__popcll(m[it] & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t c = s_cnt[it * 4 + w];
            if ((uint32_t)w < wave) j += c;
            run += c;
        }
        if (!live[it] || j >= cap) continue;
        uint32_t r[12];
        load_record(S, (uint32_t)(s0 + (uint64_t)it * 256), r);
        proj_fill_column(s_k, tid, r);
        uint32_t v4 = 0;  // bit f: IP field f of this flow is IPv4
        if constexpr (PX) {
#pragma unroll
            for (int f = 0; f < 2; f++)  // SrcIP, DstIP: a key of <= 37 bytes holds two IP fields at most
                if (pl.ipoff[f] != 0xFFu) {
                    v4 |= (px_is_v4(s_k, tid, pl.ipoff[f]) ? 1u : 0u) << f;  // the To16 value's class
                    spr_encode_ip(s_k, tid, pl.ipoff[f]);
                }
        } else {
            // the fields as a count and a list (the order does not matter: they are rewritten
            // independently): with the loop above the byte-store instantiation spills 114 SGPRs
            // instead of 112, and this form keeps both plain instantiations the code they were
#pragma unroll
            for (int f = 0; f < 2; f++)
                if ((uint32_t)f < pl.nip) spr_encode_ip(s_k, tid, pl.iplist[f]);
        }
        proj_store_row<PX, WORDS>(s_k, tid, s_t, v4, pl.Kf, flows + j * pl.Kf);
        proj_store_row<PX, WORDS>(s_k, tid, s_t + SprPlan<PX>::kRow, v4, pl.Ke, elems + j * pl.Ke);
    }
}

// epoch wrap: every live tag of a table becomes 1, older than every epoch the new generation hands out
__global__ __launch_bounds__(256) void k_exs_retag(uint32_t *rec, uint64_t slots, uint32_t RW) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < slots && rec[s * RW] != 0u) rec[s * RW] = 1u;
}

// flow-table growth: spread[] follows each record to its new slot (gns_dict.hip remap)
__global__ __launch_bounds__(256) void k_exs_permute(const uint32_t *spread, uint64_t slots, const uint32_t *remap,
                                                     uint32_t *out) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const uint32_t t = remap[s];
    if (t < kDictMarked) out[t] = spread[s];
}

__global__ __launch_bounds__(256) void k_exs_iota(uint32_t *ids, uint64_t n) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < n) ids[s] = (uint32_t)s;
}

__global__ __launch_bounds__(256) void k_exs_query(const uint8_t *flows, uint32_t stride, uint64_t n, DictDev F,
                                                   const uint32_t *spread, uint64_t *out) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    uint32_t kw[GNS_KWMAX];
    load_key_bytes<GNS_KWMAX>(flows + p * stride, F.K, false, kw);
    const uint32_t id = dict_lookup(F, kw);
    out[p] = id != GNS_ID_NONE ? (uint64_t)spread[id] : 0ull;
}

// snapshot: the occupied flow slots (at most cap; the host knows the exact count)
__global__ __launch_bounds__(256) void k_exs_list(DictDev F, uint64_t slots, uint32_t *ids, uint32_t cap, uint32_t *count) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = s < slots && F.rec[s * F.RW] != 0u;
    const uint64_t m = __ballot(live);
    if (m == 0) return;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    const uint32_t j = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (live && j < cap) ids[j] = (uint32_t)s;
}

__global__ __launch_bounds__(256) void k_exs_gather(const uint32_t *ids, uint64_t n, DictDev F, const uint32_t *spread,
                                                    uint8_t *keys, uint32_t *vals) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t id = ids[p];
    uint32_t r[12];
    load_record(F, id, r);
    for (uint32_t j = 0; j < F.K; j++) keys[p * F.K + j] = (uint8_t)(r[1 + (j >> 2)] >> (8 * (j & 3)));
    vals[p] = spread[id];
}

}  // namespace gns

// ===========================================================================
// Host side
// ===========================================================================
using namespace gns;

struct gns_exs {
    int device = 0;
    hipStream_t stream = nullptr;
    KeyPlanN kpf{}, kpm{};
    uint32_t Kf = 0, Km = 0;
    bool has_layout = false;     // tuples / headers need the field layouts
    PairDev P{};
    DictDev F{};
    uint64_t pslots = 0, fslots = 0;
    uint64_t pclaimed = 0, fclaimed = 0;  // claimed slots as of the last batch
    uint32_t *spread = nullptr;  // [fslots]
    uint32_t *ident = nullptr;   // [fslots] = slot: the rebuild's mark list and the heavy list's ids
    uint32_t *ctl = nullptr;     // [0..1] flow table claimed / abort (DictDev.ctl), [4] flow, [5] pair claims
    uint32_t *ptotal = nullptr;  // [2] parked totals (ping-pong)
    uint64_t *pend[2] = {nullptr, nullptr};
    uint32_t *pcnt[2] = {nullptr, nullptr};
    unsigned long long *stats = nullptr;
    uint32_t *h_pin = nullptr;
    uint32_t epoch = 0;          // of the last launch; record tags are claim epochs
    uint32_t gen = 1;            // cursor generation: a reset or an epoch wrap starts a new one
    uint8_t *xbuf = nullptr;     // export / merge_from staging: kExsStageRows rows of flow and element bytes
    uint64_t bmax = 0, pkt = 0, n_batches = 0;
    uint64_t n_fgrow = 0, n_pgrow = 0;
    double grow_ms = 0.0;
    DictScratch dsc;
    HostStage stage;
    CompactInput compact;        // compact records: the staged side array, the 16-byte form's sizes
    QueryStage qs;               // host queries' keys and answers on the device
    StageTimer timer;
    HhScratch hh;
};

namespace {

void exs_free_all(gns_exs *h) {
    dfree(h->P.rec); dfree(h->F.rec); dfree(h->spread); dfree(h->ident); dfree(h->ctl); dfree(h->ptotal);
    dfree(h->pend[0]); dfree(h->pend[1]); dfree(h->pcnt[0]); dfree(h->pcnt[1]); dfree(h->stats); h->stage.free_all();
    h->compact.free_all();
    h->qs.free_all();
    dfree(h->xbuf);
    h->dsc.free_all();
    h->hh.free_all();
    if (h->h_pin) (void)hipHostFree(h->h_pin);
    h->timer.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

// empty tables (create, reset); the tables keep the size they have grown to
int exs_clear(gns_exs *h) {
    hipStream_t s = h->stream;
    GNS_HIP(hipMemsetAsync(h->P.rec, 0, h->pslots * h->P.RW * 4, s));
    GNS_HIP(hipMemsetAsync(h->F.rec, 0, h->fslots * h->F.RW * 4, s));
    GNS_HIP(hipMemsetAsync(h->spread, 0, h->fslots * 4, s));
    GNS_HIP(hipMemsetAsync(h->ctl, 0, 32, s));
    h->pclaimed = h->fclaimed = 0;
    return GNS_OK;
}

unsigned exs_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }

// The pair table's hash seed, another for every handle and after every reset.  An
// export walks a table in slot order, that is in the order of its hash: rows
// merged into a table under the SAME seed would arrive sorted by home slot, each
// launch would fill one dense window, and most lanes would meet a slot claimed in
// their own launch and park, one probe step per resolve round.  Under another seed
// the exported rows are as scattered as traffic is.
uint32_t exs_fresh_seed() {
    static std::atomic<uint32_t> k{0};
    return 0x9E3779B9u + 0x632BE5ABu * k.fetch_add(1, std::memory_order_relaxed);
}

int exs_alloc_flow_side(uint64_t slots, hipStream_t s, uint32_t **spread, uint32_t **ident) {
    *spread = *ident = nullptr;
    int rc;
    if ((rc = dalloc_t(spread, slots)) || (rc = dalloc_t(ident, slots))) {
        dfree(*spread);
        *spread = nullptr;
        return rc;
    }
    hipError_t e = hipMemsetAsync(*spread, 0, slots * 4, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_exs_iota, dim3(exs_grid(slots)), dim3(256), 0, s, *ident, slots);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        dfree(*spread); dfree(*ident);
        *spread = *ident = nullptr;
        set_error("spread flow state: %s", hipGetErrorString(e));
        return GNS_E_HIP;
    }
    return GNS_OK;
}

int exs_grow_pairs(gns_exs *h, uint64_t new_slots) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = h->stream;
    PairDev N = h->P;
    GNS_TRY(dalloc_t(&N.rec, new_slots * N.RW));
    N.mask = (uint32_t)(new_slots - 1);
    hipError_t e = hipMemsetAsync(N.rec, 0, new_slots * N.RW * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->ptotal, 0, 8, s);
    if (e == hipSuccess) {
        if (h->Km <= 32) hipLaunchKernelGGL(k_exs_rehash<8>, dim3(exs_grid(h->pslots)), dim3(256), 0, s, h->P, h->pslots, N, h->ptotal);
        else hipLaunchKernelGGL(k_exs_rehash<20>, dim3(exs_grid(h->pslots)), dim3(256), 0, s, h->P, h->pslots, N, h->ptotal);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h->h_pin, h->ptotal, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || h->h_pin[0]) {
        dfree(N.rec);
        set_error("pair table growth: %s", e != hipSuccess ? hipGetErrorString(e) : "records lost");
        return GNS_E_HIP;
    }
    dfree(h->P.rec);
    h->P = N;
    h->pslots = new_slots;
    h->n_pgrow++;
    h->grow_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GNS_OK;
}

int exs_grow_flows(gns_exs *h, uint64_t new_slots) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = h->stream;
    uint32_t *nspread = nullptr, *nident = nullptr;
    GNS_TRY(exs_alloc_flow_side(new_slots, s, &nspread, &nident));
    const uint64_t old_slots = h->fslots;
    DictIds all{h->ident, old_slots};  // every occupied record is a live flow
    uint64_t slots = old_slots, live = 0;
    const int rc = dict_rebuild(h->F, slots, &all, 1, nullptr, nullptr, 0, new_slots, s, h->dsc, &live, nullptr);
    if (rc != GNS_OK) { dfree(nspread); dfree(nident); return rc; }
    hipLaunchKernelGGL(k_exs_permute, dim3(exs_grid(old_slots)), dim3(256), 0, s, h->spread, old_slots, h->dsc.remap, nspread);
    GNS_HIP(hipGetLastError());
    GNS_HIP(hipStreamSynchronize(s));
    dfree(h->spread); dfree(h->ident);
    h->spread = nspread;
    h->ident = nident;
    h->fslots = slots;
    h->fclaimed = live;
    h->n_fgrow++;
    h->grow_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GNS_OK;
}

// Both tables take the m claims the next batch can make at most, at a load of
// at most 3/4 (grown to at most 1/2).
int exs_reserve(gns_exs *h, uint64_t m) {
    const uint64_t need_p = h->pclaimed + m, need_f = h->fclaimed + m;
    if (need_p > h->pslots - h->pslots / 4) {
        uint64_t ns = h->pslots;
        while (need_p > ns / 2) ns *= 2;
        if (ns > kExsMaxPairSlots) {
            set_error("pair table: %llu pairs exceed the device (%llu-slot limit)", (unsigned long long)need_p,
                      (unsigned long long)kExsMaxPairSlots);
            return GNS_E_OOM;
        }
        ScopedStage st(h->timer, 2);
        GNS_TRY(exs_grow_pairs(h, ns));
    }
    if (need_f > h->fslots - h->fslots / 4) {
        uint64_t ns = h->fslots;
        while (need_f > ns / 2) ns *= 2;
        if (ns > kDictMaxSlots) {
            set_error("flow table: %llu flows exceed the device (%llu-slot limit)", (unsigned long long)need_f,
                      (unsigned long long)kDictMaxSlots);
            return GNS_E_OOM;
        }
        ScopedStage st(h->timer, 2);
        GNS_TRY(exs_grow_flows(h, ns));
    }
    return GNS_OK;
}

// The epoch of the next launch.  Tags are compared with cursors (newer than) and
// with the live epoch (claimed in this launch), so the 32-bit epoch must never come
// round to tags still in the tables: before it would wrap, every live tag is
// rewritten to 1, the epoch restarts at 2 and a new cursor generation begins.
int exs_next_epoch(gns_exs *h, uint32_t *out) {
    if (h->epoch == 0xFFFFFFFFu) {
        hipLaunchKernelGGL(k_exs_retag, dim3(exs_grid(h->pslots)), dim3(256), 0, h->stream, h->P.rec, h->pslots, h->P.RW);
        hipLaunchKernelGGL(k_exs_retag, dim3(exs_grid(h->fslots)), dim3(256), 0, h->stream, h->F.rec, h->fslots, h->F.RW);
        GNS_HIP(hipGetLastError());
        h->epoch = 1;
        h->gen++;
    }
    *out = ++h->epoch;
    return GNS_OK;
}

// merge: the rows are a pair set (gns_pairs_merge): the traffic counters stay
template <int KIND, int MF, int MM, int NW>
int exs_run_batch(gns_exs *h, const InputDesc &in, uint64_t n, bool merge) {
    hipStream_t s = h->stream;
    ScopedStage total_stage(h->timer, 5);
    const uint32_t nch = (uint32_t)((n + kExsChunk - 1) / kExsChunk);
    ExsArgs a{};
    a.in = in; a.n = n; a.kpf = h->kpf; a.kpm = h->kpm; a.Kf = h->Kf; a.Km = h->Km;
    a.P = h->P; a.F = h->F; a.spread = h->spread; a.nclaim = h->ctl + 4; a.stats = h->stats;
    a.merge = merge ? 1u : 0u;
    GNS_HIP(hipMemsetAsync(h->ptotal, 0, 8, s));
    int cur = 0;  // the parked list the next round reads
    for (int round = 0;; round++) {
        GNS_TRY(exs_next_epoch(h, &a.epoch));
        if (round == 0) {
            ScopedStage st(h->timer, 0);
            a.pend_out = h->pend[0]; a.cnt_out = h->pcnt[0]; a.total_out = h->ptotal;
            hipLaunchKernelGGL((k_exs_pass<KIND, MF, MM, NW, true>), dim3(nch), dim3(kExsThreads), 0, s, a);
            GNS_HIP(hipGetLastError());
            continue;  // the first resolve round is queued blind (an empty parked list makes it a no-op)
        }
        {
            ScopedStage st(h->timer, 1);
            a.pend_in = h->pend[cur]; a.cnt_in = h->pcnt[cur];
            a.pend_out = h->pend[cur ^ 1]; a.cnt_out = h->pcnt[cur ^ 1]; a.total_out = h->ptotal + (cur ^ 1);
            hipLaunchKernelGGL((k_exs_pass<KIND, MF, MM, NW, false>), dim3(nch), dim3(kExsThreads), 0, s, a);
            GNS_HIP(hipGetLastError());
            cur ^= 1;
        }
        CtlRead rd;  // the batch's one host round trip: still parked, claims, the cannot-happen word
        rd.add(h->ptotal + cur, 4, 0);
        rd.add(h->ctl + 4, 8, 1);
        rd.add(h->stats + 3, 8, 4);
        GNS_HIP(ctl_read(rd, h->h_pin, s));
        GNS_HIP(hipStreamSynchronize(s));
        h->fclaimed = h->h_pin[1];
        h->pclaimed = h->h_pin[2];
        if (h->h_pin[4] | h->h_pin[5]) {
            set_error("spread tables: a probe found no free slot (%llu pair / %llu flow slots)",
                      (unsigned long long)h->pslots, (unsigned long long)h->fslots);
            return GNS_E_FULL;
        }
        if (h->h_pin[0] == 0) break;
        if (round > 65536) { set_error("spread resolve did not converge"); return GNS_E_HIP; }
        GNS_HIP(hipMemsetAsync(h->ptotal + (cur ^ 1), 0, 4, s));
    }
    if (!merge) {
        h->pkt += n;
        h->n_batches++;
    }
    return GNS_OK;
}

template <int KIND>
int exs_batch(gns_exs *h, const InputDesc &d, uint64_t m, bool merge = false) {
    if (m == 0) return GNS_OK;
    GNS_TRY(exs_reserve(h, m));
    const bool narrow = h->Km <= 32;
    if constexpr (KIND == IN_KEYS) {
        return narrow ? exs_run_batch<KIND, PLAN_GENERIC, PLAN_GENERIC, 8>(h, d, m, merge)
                      : exs_run_batch<KIND, PLAN_GENERIC, PLAN_GENERIC, 20>(h, d, m, merge);
    } else if (plan_mode(h->kpf) == PLAN_SLICE0 && plan_mode(h->kpm) == PLAN_SLICE0) {
        return narrow ? exs_run_batch<KIND, PLAN_SLICE0, PLAN_SLICE0, 8>(h, d, m, merge)
                      : exs_run_batch<KIND, PLAN_SLICE0, PLAN_SLICE0, 20>(h, d, m, merge);
    } else {
        return narrow ? exs_run_batch<KIND, PLAN_GENERIC, PLAN_GENERIC, 8>(h, d, m, merge)
                      : exs_run_batch<KIND, PLAN_GENERIC, PLAN_GENERIC, 20>(h, d, m, merge);
    }
}

template <int KIND>
int exs_insert(gns_exs *h, InputDesc in, uint64_t n, gns_mem where, bool merge = false) {
    GNS_TRY(set_device(h->device));
    for (uint64_t off = 0; off < n; off += h->bmax) {
        const uint64_t m = std::min<uint64_t>(h->bmax, n - off);
        InputDesc d = advance(in, off);
        if (where != GNS_MEM_DEVICE) {  // stage the piece on the device
            StageList l;
            stage_input(l, d, m);
            GNS_TRY(h->stage.copy(l, h->stream));
        }
        if constexpr (KIND == IN_REC16) GNS_TRY(h->compact.unpack_sizes(d, m, h->stream));
        GNS_TRY(exs_batch<KIND>(h, d, m, merge));
    }
    return GNS_OK;
}

// --- pair set export and union ---------------------------------------------
constexpr uint64_t kExsPiece = 1ull << 20;  // slots per staged piece: the scratch does not grow with the table

uint64_t exs_cursor(const gns_exs *h) { return (uint64_t)h->gen << 32 | h->epoch; }

// `since` names a point of this handle's stream in its current generation (0: the beginning)
int exs_check_since(const gns_exs *h, uint64_t since) {
    if (since == 0) return GNS_OK;
    if ((uint32_t)(since >> 32) != h->gen || (uint32_t)since > h->epoch) {
        set_error("cursor %llx is not of this handle's generation %u (reset, epoch wrap or another handle): take a full "
                  "export (since = 0)", (unsigned long long)since, h->gen);
        return GNS_E_ARG;
    }
    return GNS_OK;
}

constexpr uint64_t kExsStageRows = 2 * kExsPiece;  // merge_from gathers pieces until more than one piece's worth is staged

// the staging buffer laid out for `rows` (<= kExsStageRows) rows: flow bytes, then (16-byte aligned) element bytes
int exs_stage_rows(gns_exs *h, uint64_t rows, uint8_t **f, uint8_t **e) {
    if (!h->xbuf) GNS_TRY(dalloc(reinterpret_cast<void **>(&h->xbuf), kExsStageRows * h->Km + 64));
    *f = h->xbuf;
    *e = h->xbuf + ((rows * h->Kf + 15) & ~15ull);
    return GNS_OK;
}

// src's live records of slots [beg, end) newer than `since`, compacted on stream s into
// rows at flows / elems (at most cap are written).  *count is zeroed first, or with `append`
// goes on from the rows already there: the new rows follow them.
int exs_export_range(const gns_exs *src, uint64_t beg, uint64_t end, uint32_t since, uint8_t *flows, uint8_t *elems,
                     uint64_t cap, uint32_t *count, hipStream_t s, bool append = false) {
    if (!append) GNS_HIP(hipMemsetAsync(count, 0, 4, s));
    const uint32_t Ke = src->Km - src->Kf;
    const bool words = src->Kf % 4 == 0 && Ke % 4 == 0 && (((uintptr_t)flows | (uintptr_t)elems) & 3u) == 0;
    const dim3 g((unsigned)((end - beg + 256 * kExsExportIt - 1) / (256 * kExsExportIt))), b(256);
    if (src->Km <= 32) {
        if (words) hipLaunchKernelGGL((k_exs_export<8, true>), g, b, 0, s, src->P, beg, end, since, src->Kf, flows, elems, cap, count);
        else hipLaunchKernelGGL((k_exs_export<8, false>), g, b, 0, s, src->P, beg, end, since, src->Kf, flows, elems, cap, count);
    } else {
        if (words) hipLaunchKernelGGL((k_exs_export<20, true>), g, b, 0, s, src->P, beg, end, since, src->Kf, flows, elems, cap, count);
        else hipLaunchKernelGGL((k_exs_export<20, false>), g, b, 0, s, src->P, beg, end, since, src->Kf, flows, elems, cap, count);
    }
    GNS_HIP(hipGetLastError());
    return GNS_OK;
}

// the count word of the last exs_export_range on h's stream (synchronizes)
int exs_read_count(gns_exs *h, uint64_t *out) {
    GNS_HIP(hipMemcpyAsync(h->h_pin + 8, h->ctl + 6, 4, hipMemcpyDeviceToHost, h->stream));
    GNS_HIP(hipStreamSynchronize(h->stream));
    *out = h->h_pin[8];
    return GNS_OK;
}

// the `staged` rows of exs_stage_rows' buffer merged into h, in device batches of h
int exs_merge_staged(gns_exs *h, const uint8_t *flows, const uint8_t *elems, uint64_t staged) {
    InputDesc in{};
    in.keys = flows; in.stride = h->Kf; in.keys2 = elems; in.stride2 = h->Km - h->Kf;
    for (uint64_t off = 0; off < staged; off += h->bmax)
        GNS_TRY(exs_batch<IN_KEYS>(h, advance(in, off), std::min(h->bmax, staged - off), true));
    return GNS_OK;
}

// --- spread roll-up ----------------------------------------------------------
// Both plans of a spread roll-up from the source's key to the destination's flow and element
// keys (pair = flow ‖ elem, the first Kf bytes the flow's): roll_tables per row, the flow row
// under fpx and the element row under epx (nullptr: no mask), laid out for the EncodeFlow form.
// GNS_E_ARG when a field of the destination is not part of the source.
int spr_make_plans(const KeyPlanN &src, const KeyPlanN &pair, uint32_t Kf, const gns_prefix *fpx, const gns_prefix *epx,
                   SprPlan<false> *pl, SprPlan<true> *pp) {
    memset(pl, 0, sizeof(*pl));
    memset(pp, 0, sizeof(*pp));
    pp->Kf = Kf;
    pp->Ke = pair.K - Kf;
    memset(pp->ipoff, 0xFF, sizeof(pp->ipoff));
    for (int r = 0; r < 2; r++) {
        const uint8_t *dst = pair.src + (r ? Kf : 0);
        RollRow row;
        const int miss = roll_tables(src.src, src.K, dst, r ? pp->Ke : Kf, r ? epx : fpx, true, &row, pp->ipoff);
        if (miss >= 0) {
            set_error("spread rollup: %s field %s is not part of the source's key layout", r ? "element" : "flow",
                      tuple_field_name(dst[miss]));
            return GNS_E_ARG;
        }
        memcpy(pp->t[r], &row, sizeof(row));
        memcpy(pl->t[r], row.g, sizeof(row.g));
    }
    pl->Kf = pp->Kf;
    pl->Ke = pp->Ke;
    for (int f = 0; f < 2; f++)
        if (pp->ipoff[f] != 0xFF) pl->iplist[pl->nip++] = pp->ipoff[f];
    return GNS_OK;
}

}  // namespace

extern "C" {

int gns_exs_create(const gns_exs_params *p, gns_exs **out) {
    if (!p || !out) { set_error("null argument"); return GNS_E_ARG; }
    *out = nullptr;
    // the layouts first: a bad one is an argument error with or without a device
    KeyPlanN kpf, kpe, kpm;
    if (p->flow.n_fields > 8 || p->elem.n_fields > 8) { set_error("layout has more than 8 fields"); return GNS_E_ARG; }
    GNS_TRY(make_plan(p->flow, p->flow_bytes, &kpf));
    GNS_TRY(make_plan(p->elem, p->elem_bytes, &kpe));
    if (kpf.K == 0 || kpe.K == 0) {
        set_error("flow key of %u bytes, element key of %u bytes: both must be 1..37", kpf.K, kpe.K);
        return GNS_E_ARG;
    }
    const bool has_layout = p->flow.n_fields && p->elem.n_fields;
    if (has_layout) {
        GNS_TRY(make_plan2(p->flow, p->elem, &kpm));
    } else {
        memset(&kpm, 0, sizeof(kpm));
        kpm.K = kpf.K + kpe.K;
        kpm.woff = -1;
    }
    if (p->max_flows > kDictMaxSlots / 2 || p->max_pairs > kExsMaxPairSlots / 2) {
        set_error("max_flows > 2^29 or max_pairs > 2^30");
        return GNS_E_ARG;
    }
    GNS_TRY(check_device(p->device));
    gns_exs *h = new gns_exs();
    h->device = p->device;
    h->kpf = kpf; h->kpm = kpm; h->Kf = kpf.K; h->Km = kpm.K; h->has_layout = has_layout;
    int rc = GNS_OK;
    do {
        if ((rc = set_device(h->device)) != GNS_OK) break;
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed"); rc = GNS_E_HIP; break;
        }
        h->timer.stream = h->stream;
        const uint64_t mf = p->max_flows ? p->max_flows : (1ull << 20);
        const uint64_t mp = p->max_pairs ? p->max_pairs : (4ull << 20);
        h->fslots = 16; h->pslots = 16;
        while (h->fslots < 2 * mf) h->fslots <<= 1;
        while (h->pslots < 2 * mp) h->pslots <<= 1;
        h->bmax = p->batch_packets ? p->batch_packets : (4ull << 20);
        h->bmax = std::min<uint64_t>(h->bmax, 1ull << 26);
        // tests: a starting epoch a few launches short of 2^32 makes the wrap reachable
        if (const char *ee = getenv("GNS_EXS_TEST_EPOCH")) h->epoch = (uint32_t)strtoull(ee, nullptr, 0);
        const uint64_t nch = (h->bmax + kExsChunk - 1) / kExsChunk;
        const uint32_t nkw = (h->Km + 3) / 4;
        h->P.RW = 1 + nkw <= 16 ? 16u : 32u;
        h->P.mask = (uint32_t)(h->pslots - 1);
        h->P.seed = exs_fresh_seed();
        h->P.K = h->Km;
        h->F.mask = (uint32_t)(h->fslots - 1);
        h->F.K = h->Kf;
        h->F.RW = dict_record_words(h->Kf);
        h->F.seed = 0x2545F491u;
        h->F.cap = 0xFFFFFFFFu;  // never reached: exs_reserve grows the table before a batch
        if ((rc = dalloc_t(&h->P.rec, h->pslots * h->P.RW)) || (rc = dalloc_t(&h->F.rec, h->fslots * h->F.RW)) ||
            (rc = exs_alloc_flow_side(h->fslots, h->stream, &h->spread, &h->ident)) ||
            (rc = dalloc_t(&h->ctl, 8)) || (rc = dalloc_t(&h->ptotal, 2)) ||
            (rc = dalloc_t(&h->pend[0], nch * kExsChunk)) || (rc = dalloc_t(&h->pend[1], nch * kExsChunk)) ||
            (rc = dalloc_t(&h->pcnt[0], nch)) || (rc = dalloc_t(&h->pcnt[1], nch)) || (rc = dalloc_t(&h->stats, 8)))
            break;
        h->F.ctl = h->ctl;
        if (hipHostMalloc(reinterpret_cast<void **>(&h->h_pin), 64, 0) != hipSuccess) {
            set_error("hipHostMalloc failed"); rc = GNS_E_OOM; break;
        }
        if (hipMemsetAsync(h->stats, 0, 64, h->stream) != hipSuccess) { rc = GNS_E_HIP; break; }
        if ((rc = exs_clear(h)) != GNS_OK) break;
        if (hipStreamSynchronize(h->stream) != hipSuccess) { set_error("create: stream error"); rc = GNS_E_HIP; break; }
    } while (0);
    if (rc != GNS_OK) {
        exs_free_all(h);
        delete h;
        return rc;
    }
    *out = h;
    return GNS_OK;
}

int gns_exs_destroy(gns_exs *h) {
    if (!h) return GNS_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    exs_free_all(h);
    delete h;
    return GNS_OK;
}

int gns_exs_insert_keys(gns_exs *h, const uint8_t *flows, uint32_t fstride, const uint8_t *elems, uint32_t estride,
                        uint64_t n, gns_mem where) {
    if (!h || (n && (!flows || !elems))) { set_error("null argument"); return GNS_E_ARG; }
    if (fstride < h->Kf || estride < h->Km - h->Kf) { set_error("stride smaller than key"); return GNS_E_ARG; }
    InputDesc in{};
    in.keys = flows; in.stride = fstride; in.keys2 = elems; in.stride2 = estride;
    return exs_insert<IN_KEYS>(h, in, n, where);
}

int gns_exs_insert_tuples(gns_exs *h, const gns_tuples *t, uint64_t n, gns_mem where) {
    if (!h || !t) { set_error("null argument"); return GNS_E_ARG; }
    if (!h->has_layout) { set_error("handle created without field layouts: keys input only"); return GNS_E_ARG; }
    if (n && (!t->src16 || !t->dst16 || !t->sport || !t->dport || !t->proto)) { set_error("null tuple array"); return GNS_E_ARG; }
    return exs_insert<IN_TUPLE>(h, tuples_desc(*t, false), n, where);
}

int gns_exs_insert_headers(gns_exs *h, const uint8_t *hdr, const uint32_t *wirelen, uint64_t n, gns_mem where) {
    if (!h || (n && (!hdr || !wirelen))) { set_error("null argument"); return GNS_E_ARG; }
    if (!h->has_layout) { set_error("handle created without field layouts: keys input only"); return GNS_E_ARG; }
    return exs_insert<IN_HDR>(h, headers_desc(hdr, wirelen), n, where);
}

int gns_spread_insert_compact(gns_exs *h, const uint8_t *rec16, const uint32_t *wirelen, uint64_t n,
                           const uint8_t *side64, uint64_t n_side, gns_mem where) {
    if (!h || (n && !rec16) || (n_side && !side64)) { set_error("null argument"); return GNS_E_ARG; }
    if (!h->has_layout) { set_error("handle created without field layouts: keys input only"); return GNS_E_ARG; }
    InputDesc in = compact_desc(rec16, wirelen, side64, n_side);
    if (where != GNS_MEM_DEVICE) {  // the resolve rounds re-read the side records: one device copy for the whole call
        GNS_TRY(set_device(h->device));
        GNS_TRY(h->compact.stage_side(in, h->stream));
    }
    return exs_insert<IN_REC16>(h, in, n, where);
}

int gns_exs_flush(gns_exs *h) {
    if (!h) return GNS_E_ARG;
    return handle_flush(h->device, h->stream, h->timer);
}

static int exs_query_impl(gns_exs *h, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out, bool dev) {
    if (!h) { set_error("null argument"); return GNS_E_ARG; }
    return query_keys(h->device, h->stream, h->qs, "spread", flows, stride, h->Kf, n, out, dev,
                      [&](const uint8_t *dk, uint64_t *dout) -> int {
                          hipLaunchKernelGGL(k_exs_query, dim3(exs_grid(n)), dim3(256), 0, h->stream, dk, stride, n, h->F,
                                             h->spread, dout);
                          return GNS_OK;
                      });
}

int gns_exs_query(gns_exs *h, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out) {
    return exs_query_impl(h, flows, stride, n, out, false);
}

int gns_exs_query_device(gns_exs *h, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out) {
    return exs_query_impl(h, flows, stride, n, out, true);
}

// The flows with spread >= threshold through the shared list code (gns_hh.hpp):
// the cell array is spread[] itself, one cell per flow-table slot, whose id is the
// slot.  A list longer than the caller's buffers is reported and not written.
int gns_exs_heavy_hitters(gns_exs *h, uint32_t threshold, uint8_t *flows, uint32_t *spreads, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    GNS_HIP(hipStreamSynchronize(h->stream));
    const uint64_t cap = *n_io;
    std::vector<uint8_t> tf(flows ? cap * h->Kf : 0);
    std::vector<uint32_t> tv(spreads ? cap : 0);
    uint64_t n = cap;
    // a seen flow has spread >= 1, so threshold 0 lists the same flows as 1 (empty slots hold 0)
    GNS_TRY(gns::hh_heavy_list(h->hh, h->stream, h->F, h->fslots, h->Kf, h->fslots, h->spread, h->ident,
                               std::max(threshold, 1u), flows ? tf.data() : nullptr, spreads ? tv.data() : nullptr, &n));
    *n_io = n;
    if (n <= cap && n) {
        if (flows) memcpy(flows, tf.data(), n * h->Kf);
        if (spreads) memcpy(spreads, tv.data(), n * 4);
    }
    return GNS_OK;
}

int gns_exs_snapshot(gns_exs *h, uint8_t *flows, uint32_t *spreads, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    hipStream_t s = h->stream;
    GNS_HIP(hipStreamSynchronize(s));
    const uint64_t cap = *n_io, nf = h->fclaimed;  // every claimed flow slot holds a seen flow
    *n_io = nf;
    if (nf == 0 || nf > cap || (!flows && !spreads)) return GNS_OK;
    uint32_t *ids = nullptr, *dv = nullptr;
    uint8_t *dk = nullptr;
    int rc;
    if ((rc = dalloc_t(&ids, nf)) || (rc = dalloc_t(&dv, nf)) || (rc = dalloc(reinterpret_cast<void **>(&dk), nf * h->Kf))) {
        dfree(ids); dfree(dv);
        return rc;
    }
    hipError_t e = hipMemsetAsync(h->ptotal, 0, 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(ids, 0, nf * 4, s);  // every id the gather reads names a slot
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_exs_list, dim3(exs_grid(h->fslots)), dim3(256), 0, s, h->F, h->fslots, ids, (uint32_t)nf, h->ptotal);
        hipLaunchKernelGGL(k_exs_gather, dim3(exs_grid(nf)), dim3(256), 0, s, ids, nf, h->F, h->spread, dk, dv);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h->h_pin, h->ptotal, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && flows) e = hipMemcpyAsync(flows, dk, nf * h->Kf, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && spreads) e = hipMemcpyAsync(spreads, dv, nf * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    dfree(ids); dfree(dv); dfree(dk);
    if (e != hipSuccess) { set_error("spread snapshot: %s", hipGetErrorString(e)); return GNS_E_HIP; }
    if (h->h_pin[0] != nf) {
        set_error("spread snapshot: %u occupied flow slots, %llu claimed", h->h_pin[0], (unsigned long long)nf);
        return GNS_E_HIP;
    }
    return GNS_OK;
}

int gns_exs_reset(gns_exs *h) {
    if (!h) return GNS_E_ARG;
    GNS_TRY(set_device(h->device));
    GNS_TRY(exs_clear(h));
    h->gen++;  // cursors taken before name pairs that are gone
    h->P.seed = exs_fresh_seed();  // restoring this handle's own export must not arrive in its hash order
    GNS_HIP(hipStreamSynchronize(h->stream));
    return GNS_OK;
}

int gns_pairs_export(gns_exs *h, uint64_t since, uint8_t *flows, uint8_t *elems, uint64_t *n, uint64_t *cursor,
                     gns_mem where) {
    if (!h || !n) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(exs_check_since(h, since));
    GNS_TRY(set_device(h->device));
    hipStream_t s = h->stream;
    const bool rows = flows && elems;
    const uint64_t cap = rows ? *n : 0, cap_in = *n;
    const uint32_t se = (uint32_t)since, Ke = h->Km - h->Kf;
    uint64_t total = 0;
    if (!rows && since == 0) {
        GNS_HIP(hipStreamSynchronize(s));
        total = h->pclaimed;  // every claimed slot holds a pair; the host knows the count as of the last batch
    } else if (!rows || where == GNS_MEM_DEVICE) {
        GNS_TRY(exs_export_range(h, 0, h->pslots, se, flows, elems, cap, h->ctl + 6, s));
        GNS_TRY(exs_read_count(h, &total));
    } else {
        for (uint64_t beg = 0; beg < h->pslots; beg += kExsPiece) {
            const uint64_t end = std::min(h->pslots, beg + kExsPiece);
            uint8_t *df, *de;
            GNS_TRY(exs_stage_rows(h, kExsPiece, &df, &de));
            GNS_TRY(exs_export_range(h, beg, end, se, df, de, kExsPiece, h->ctl + 6, s));
            uint64_t c = 0;
            GNS_TRY(exs_read_count(h, &c));
            const uint64_t w = total < cap ? std::min(c, cap - total) : 0;
            if (w) {
                GNS_HIP(hipMemcpy(flows + total * h->Kf, df, w * h->Kf, hipMemcpyDeviceToHost));
                GNS_HIP(hipMemcpy(elems + total * Ke, de, w * Ke, hipMemcpyDeviceToHost));
            }
            total += c;
        }
    }
    *n = total;
    if (cursor && total <= cap_in && (rows || total == 0)) *cursor = exs_cursor(h);
    return GNS_OK;
}

int gns_pairs_merge(gns_exs *h, const uint8_t *flows, uint32_t fstride, const uint8_t *elems, uint32_t estride,
                    uint64_t n, gns_mem where) {
    if (!h || (n && (!flows || !elems))) { set_error("null argument"); return GNS_E_ARG; }
    if (fstride < h->Kf || estride < h->Km - h->Kf) { set_error("stride smaller than key"); return GNS_E_ARG; }
    InputDesc in{};
    in.keys = flows; in.stride = fstride; in.keys2 = elems; in.stride2 = estride;
    return exs_insert<IN_KEYS>(h, in, n, where, true);
}

int gns_pairs_merge_from(gns_exs *dst, gns_exs *src, uint64_t since, uint64_t *cursor) {
    if (!dst || !src) { set_error("null argument"); return GNS_E_ARG; }
    if (dst == src) { set_error("merge_from: source and destination are the same handle"); return GNS_E_ARG; }
    if (dst->Kf != src->Kf || dst->Km != src->Km) {
        set_error("merge_from: key sizes differ (%u + %u bytes into %u + %u)", src->Kf, src->Km - src->Kf, dst->Kf,
                  dst->Km - dst->Kf);
        return GNS_E_ARG;
    }
    if (dst->device != src->device) { set_error("merge_from: handles on devices %d and %d", src->device, dst->device); return GNS_E_ARG; }
    GNS_TRY(exs_check_since(src, since));
    GNS_TRY(set_device(dst->device));
    // src is read at this point of its own stream, by kernels on dst's stream
    GNS_TRY(stream_wait_now(dst->stream, src->stream, "merge_from"));
    const uint64_t at = exs_cursor(src);
    // Pieces of src's table are compacted one behind the other into the staging rows; once more
    // than one piece's worth is staged (the next piece might not fit) they are merged, in device
    // batches of dst.  A sparse table thus still merges batches of 2^20 rows or more.
    uint8_t *df, *de;
    GNS_TRY(exs_stage_rows(dst, kExsStageRows, &df, &de));
    uint64_t staged = 0;
    for (uint64_t beg = 0; beg < src->pslots; beg += kExsPiece) {
        const uint64_t end = std::min(src->pslots, beg + kExsPiece);
        GNS_TRY(exs_export_range(src, beg, end, (uint32_t)since, df, de, kExsStageRows, dst->ctl + 6, dst->stream, staged != 0));
        GNS_TRY(exs_read_count(dst, &staged));
        if (staged <= kExsPiece && end < src->pslots) continue;
        GNS_TRY(exs_merge_staged(dst, df, de, staged));
        staged = 0;
    }
    if (cursor) *cursor = at;
    return GNS_OK;
}

namespace {
// gns_spread_rollup (no prefixes) and gns_spread_rollup_prefix behind their argument checks
static int spr_rollup(gns_exs *dst, gns_ex *src, const gns_prefix *fpx, const gns_prefix *epx, uint64_t since, uint64_t *cursor,
               uint64_t out[2]) {
    if (!dst->has_layout) {
        set_error("spread rollup: dst was created without field layouts (key sizes only): nothing names the fields to project");
        return GNS_E_ARG;
    }
    ExTableRef S;
    ex_table_ref(src, &S);
    SprPlan<false> pl;
    SprPlan<true> pp;
    GNS_TRY(spr_make_plans(S.kp, dst->kpm, dst->Kf, fpx, epx, &pl, &pp));
    if (dst->device != S.device) {
        set_error("spread rollup: dst is on device %d, src on device %d", dst->device, S.device);
        return GNS_E_ARG;
    }
    if (since > S.pos) {
        set_error("spread rollup: since %llu is beyond src's stream position %llu", (unsigned long long)since,
                  (unsigned long long)S.pos);
        return GNS_E_ARG;
    }
    GNS_TRY(set_device(dst->device));
    const uint64_t piece = test_piece("GNS_SPREAD_ROLLUP_PIECE", kExsPiece);
    hipStream_t s = dst->stream;
    // src is read at this point of its own stream (after its pending batches), by kernels on dst's stream
    GNS_TRY(stream_wait_now(s, S.stream, "spread rollup"));
    // Pieces of src's table are projected one behind the other into the staging rows; once more
    // than one piece's worth of rows is staged (the next piece might not fit: a piece appends at
    // most `piece` rows, and the buffer holds two pieces of 2^20) they are merged, in device
    // batches of dst.
    uint8_t *df, *de;
    GNS_TRY(exs_stage_rows(dst, kExsStageRows, &df, &de));
    const bool words = dst->Kf % 4 == 0 && (dst->Km - dst->Kf) % 4 == 0 && (((uintptr_t)df | (uintptr_t)de) & 3u) == 0;
    const uint64_t pairs0 = dst->pclaimed;
    uint64_t staged = 0, projected = 0;
    for (uint64_t beg = 0; beg < S.slots; beg += piece) {
        const uint64_t end = std::min(S.slots, beg + piece);
        if (staged == 0) GNS_HIP(hipMemsetAsync(dst->ctl + 6, 0, 4, s));
        {
            ScopedStage st(dst->timer, 3);
            const dim3 g((unsigned)((end - beg + 256 * kSprIt - 1) / (256 * kSprIt))), b(256);
            auto launch = [&](auto kernel, const auto &plan) {
                hipLaunchKernelGGL(kernel, g, b, 0, s, S.D, S.pkts, S.first, beg, end, (unsigned long long)since, plan, df, de,
                                   kExsStageRows, dst->ctl + 6);
            };
            if (fpx) launch(words ? k_spr_project<true, true> : k_spr_project<true, false>, pp);
            else launch(words ? k_spr_project<false, true> : k_spr_project<false, false>, pl);
            GNS_HIP(hipGetLastError());
        }
        GNS_TRY(exs_read_count(dst, &staged));
        staged = std::min(staged, kExsStageRows);  // (rows past the capacity are counted, not written: cannot happen)
        if (staged <= piece && end < S.slots) continue;
        GNS_TRY(exs_merge_staged(dst, df, de, staged));
        projected += staged;
        staged = 0;
    }
    if (cursor) *cursor = S.pos;
    if (out) { out[0] = projected; out[1] = dst->pclaimed - pairs0; }
    return GNS_OK;
}
}  // namespace

int gns_spread_rollup(gns_exs *dst, gns_ex *src, uint64_t since, uint64_t *cursor, uint64_t out[2]) {
    if (!dst || !src) { set_error("null argument"); return GNS_E_ARG; }
    return spr_rollup(dst, src, nullptr, nullptr, since, cursor, out);
}

int gns_spread_rollup_prefix(gns_exs *dst, gns_ex *src, const gns_prefix *flow_px, const gns_prefix *elem_px,
                             uint64_t since, uint64_t *cursor, uint64_t out[2]) {
    if (!dst || !src) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(px_check_prefix(flow_px, "spread rollup"));
    GNS_TRY(px_check_prefix(elem_px, "spread rollup"));
    return spr_rollup(dst, src, flow_px, elem_px, since, cursor, out);
}

int gns_exs_counters(gns_exs *h, uint64_t out[8]) {
    if (!h || !out) return GNS_E_ARG;
    GNS_TRY(set_device(h->device));
    GNS_HIP(hipStreamSynchronize(h->stream));
    unsigned long long st[8];
    GNS_HIP(hipMemcpy(st, h->stats, sizeof(st), hipMemcpyDeviceToHost));
    out[0] = st[0]; out[1] = st[1]; out[2] = st[2]; out[3] = st[3]; out[4] = st[4];
    out[5] = h->fclaimed; out[6] = h->pkt; out[7] = h->n_batches;
    return GNS_OK;
}

int gns_exs_dict_stats(gns_exs *h, uint64_t out[8]) {
    if (!h || !out) return GNS_E_ARG;
    out[0] = h->n_fgrow; out[1] = h->n_pgrow; out[2] = h->fslots; out[3] = h->fclaimed;
    out[4] = h->pslots; out[5] = h->pclaimed; out[6] = (uint64_t)(h->grow_ms * 1000.0); out[7] = 0;
    return GNS_OK;
}

int gns_exs_set_timing(gns_exs *h, int on) {
    if (!h) return GNS_E_ARG;
    set_timing_arg(h->timer, on);
    return GNS_OK;
}

int gns_exs_stage_times(gns_exs *h, double ms[8], uint64_t launches[8], int reset) {
    if (!h) return GNS_E_ARG;
    GNS_TRY(set_device(h->device));
    h->timer.report(ms, launches, reset);
    return GNS_OK;
}

}  // extern "C"
