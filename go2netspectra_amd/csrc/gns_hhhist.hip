// gns_hhhist.hip -- the heavy-hitter history (gns_hh_hist_*): the store behind
// QueryHeavyHitters' EndTime (internal/query/querier.go:191-248).  The reference's sketch
// writer appends one row (Timestamp, TaskName, Flow, Value, Type) per list entry of every
// interval's Snapshot() (internal/engine/impl/sketch/writer_clickhouse.go:86-138) and the
// query takes, per Flow, argMax(Value, Timestamp) over the rows of one Type with
// Timestamp <= EndTime.  Here that table lives on the device:
//   - one key index of the history's own (HistIndex, gns_histindex.hpp), a dictionary of K-byte
//     flows shared by all types;
//   - per type a LANE: a log of 16-byte rows {index slot, value, written, superseded} and one
//     head word per index slot, the newest log row of that (type, flow).  Key bytes live only
//     in the index.  written / superseded are snapshot numbers as in the exact history
//     (gns_exact.hip): a row is live as of snapshot s when written <= s < superseded.
// The timestamp table and s(T) are the host's (gns_hhplan.hpp over gns_histplan.hpp).
//   A1  HistIndex::resolve  packed rows [flow | u32] at stride K + 4 -> index slots, piece by
//                           piece; a growth renumbers the head words and k_hhh_reslot the logs
//   A1b ::check_unique      no two rows of one list in one index slot (over the whole list)
//   A2  k_hhh_link          list row i -> lane row base + i, swapped into the head word; the
//                           row it displaced is stamped superseded = S
//   Q1  k_hhh_hist / _pick  limit != 0: a three-level radix select (11 + 11 + 10 bits) over
//                           the live values fixes the cut value v*, the largest value with at
//                           least `limit` live rows at or above it
//   Q2  k_hhh_collect       live rows with value >= max(threshold, v*) -> packed rows
//                           [flow | u32], key bytes from the index record
//   Q3  hh_order_rows_dev   the canonical order (gns_hh.hip), then the cut to `limit`
//   T1  k_hhh_trim_count    gns_hh_hist_trim, per lane: the rows of each 256-row block of the
//                           expired prefix that a fold keeps
//   T2  k_hhh_scan / _add   the exclusive scan of the block counts, 1,024 per workgroup and level
//   T3  k_hhh_trim_move     the kept rows, stably, into a new log; k_hhh_trim_heads then reads
//                           the new head words off it (the newest row of a slot is its open one)
//   P1  k_hhh_q_lookup      gns_hh_hist_query: flows -> index slots (dict_lookup: no insert);
//                           as of the newest snapshot the head word answers
//   P2  ::own / k_hhh_q_scan as of an older one: one pass over the lane's rows answers for the
//                           live row of every wanted slot; P3 k_hhh_q_dup copies to duplicates
// A fold keeps one row per (type, flow) pair ever listed, because the store has no tombstones: it
// bounds the log by snapshots x list length + distinct pairs.  Only a drop bounds the index.
// Not offered: roll-ups.
// Everything an append writes before the host publishes the snapshot lies outside every scan:
// rows at and beyond a lane's published count, and superseded words that equal the new S.
#include <mutex>
#include <vector>

#include "gns_common.hpp"
#include "gns_hh.hpp"
#include "gns_hhplan.hpp"
#include "gns_histindex.hpp"

namespace gns {

namespace {
constexpr uint32_t kSelBins = 2048;  // bins of one select level (LDS: 8 KB)

// A2.  rows: packed [flow (K) | u32 LE value] at stride K + 4 (any alignment).
__global__ __launch_bounds__(256) void k_hhh_link(const uint8_t *rows, uint32_t K, uint64_t n, const uint32_t *ids,
                                                  uint32_t *head, uint32_t slots, uint4 *log, uint64_t cap, uint64_t base,
                                                  uint32_t S, uint32_t *fresh) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t r = base + i;
    bool isnew = false;
    if (i < n && r < cap) {
        const uint32_t id = ids[i];
        if (id < slots) {  // (always: every id of the append was resolved before the link)
            const uint8_t *p = rows + i * (uint64_t)(K + 4) + K;
            const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            log[r] = make_uint4(id, v, S, kHistOpen);
            const uint32_t old = head[id];
            head[id] = (uint32_t)r;
            if (old == kHistOpen) isnew = true;
            else if (old < base) log[old].w = S;
        }
    }
    const uint64_t m = __ballot(isnew);  // (type, flow) pairs new to the lane: one add per wave
    if (m && __lane_id() == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(fresh, (uint32_t)__popcll(m));
}

// index growth: a log row's slot follows its record (HistIndex::grow's remap)
__global__ __launch_bounds__(256) void k_hhh_reslot(uint4 *log, uint64_t rows, uint64_t slots, const uint32_t *remap) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint32_t id = log[r].x;
    if (id < slots) log[r].x = remap[id];  // (a published row's slot is marked: its key has a head word)
}

// a row is live as of snapshot s
__device__ __forceinline__ bool hhh_live(const uint4 &q, uint32_t s) { return q.z <= s && s < q.w; }

// gns_hh_hist_trim, lane by lane.  Of the expired prefix [0, R) of a lane's log the rows still
// live as of the last expired snapshot s_last stay under a fold (superseded > s_last), none under
// a drop; every row from R on stays.  T1 counts the staying rows of each 256-row block of the
// prefix, T2 scans the counts, T3 moves the rows stably into the new log G: a prefix row to its
// rank, a later row to r - R + nbase.  Version words lose d; a written word below d belongs to
// the base and becomes 0.  The old log is only read: a failed trim leaves it as it was.
struct HhTrim {
    uint64_t rows, R, nbase, row0, cap;  // row0: the first row of T3's grid (0 when the prefix is ranked)
    uint32_t s_last, d;
    int fold;
};
__global__ __launch_bounds__(256) void k_hhh_trim_count(const uint4 *log, uint64_t R, uint32_t s_last, uint32_t *cnt) {
    __shared__ uint32_t s_w[4];
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool sel = r < R && log[r].w > s_last;
    const uint64_t m = __ballot(sel);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// T2: a[0, n) -> its exclusive scan in place, 1,024 words per workgroup; the workgroup's sum goes
// to sums[blockIdx.x] (the host scans those in turn and k_hhh_scan_add adds them back)
constexpr uint32_t kScanTile = 1024;
__global__ __launch_bounds__(256) void k_hhh_scan(uint32_t *a, uint64_t n, uint32_t *sums) {
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + 4u * tid;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        v[j] = i0 + j < n ? a[i0 + j] : 0u;
        sum += v[j];
    }
    uint32_t inc = sum;  // inclusive scan over the wave
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t x = __shfl_up(inc, o);
        if (lane >= o) inc += x;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (uint32_t w = 0; w < wave; w++) run += s_w[w];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (i0 + j < n) a[i0 + j] = run;
        run += v[j];
    }
    if (tid == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ __launch_bounds__(256) void k_hhh_scan_add(uint32_t *a, uint64_t n, const uint32_t *sums) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] += sums[i / kScanTile];
}
// T3.  off: T2's scan of T1's counts (block b of this grid is T1's block b); nullptr: no prefix row stays
__global__ __launch_bounds__(256) void k_hhh_trim_move(const uint4 *O, HhTrim t, const uint32_t *off, uint4 *G) {
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t r = t.row0 + (uint64_t)blockIdx.x * 256 + tid;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (r < t.rows) q = O[r];
    const bool prefix = r < t.R;
    const bool sel = prefix && t.fold && q.w > t.s_last;
    const uint64_t m = __ballot(sel);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (r >= t.rows || (prefix && !sel)) return;
    uint64_t nr = r - t.R + t.nbase;
    if (prefix) {
        nr = off[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; w++) nr += s_w[w];
    }
    if (nr >= t.cap) return;
    G[nr] = make_uint4(q.x, q.y, max(q.z, t.d) - t.d, q.w == kHistOpen ? kHistOpen : q.w - t.d);
}
// The newest row of a (lane, slot) is the slot's only row that nothing superseded: the head words
// of a new log, into an array cleared to kHistOpen
__global__ __launch_bounds__(256) void k_hhh_trim_heads(const uint4 *log, uint64_t rows, uint64_t slots, uint32_t *nh) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const uint4 q = log[r];
    if (q.w == kHistOpen && q.x < slots) nh[q.x] = (uint32_t)r;
}
// (type, flow) pairs a trim forgets: the old head word names a row, the new one none
__global__ __launch_bounds__(256) void k_hhh_trim_forgot(const uint32_t *oh, const uint32_t *nh, uint64_t slots,
                                                         uint32_t *forgot) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool gone = s < slots && oh[s] != kHistOpen && nh[s] == kHistOpen;
    const uint64_t m = __ballot(gone);
    if (m && __lane_id() == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(forgot, (uint32_t)__popcll(m));
}
// the keys some lane still names (HistIndex::mark_heads' list)
__global__ __launch_bounds__(256) void k_hhh_trim_named(const uint32_t *ids, uint64_t slots, uint32_t *named) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t m = __ballot(s < slots && ids[s] != GNS_ID_NONE);
    if (m && __lane_id() == (uint32_t)(__ffsll((unsigned long long)m) - 1)) atomicAdd(named, (uint32_t)__popcll(m));
}

// gns_hh_hist_query.  P1: flow i -> its index slot (a read-only lookup: nothing is claimed) and
// the answer "no live row"; as of the newest snapshot the lane's head word names the live row.
__global__ __launch_bounds__(256) void k_hhh_q_lookup(const uint8_t *flows, uint64_t n, DictDev D, const uint32_t *head,
                                                      const uint4 *log, uint64_t rows, uint32_t *ids,
                                                      unsigned long long *values, uint8_t *found) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t kw[GNS_KWMAX];
    load_key_bytes<GNS_KWMAX>(flows + i * D.K, D.K, false, kw);
    const uint32_t id = dict_lookup(D, kw);
    ids[i] = id;
    unsigned long long v = 0;
    uint8_t f = 0;
    if (head && id != GNS_ID_NONE) {
        const uint32_t r = head[id];
        if (r < rows) { v = log[r].y; f = 1; }  // (kHistOpen lies beyond every log)
    }
    values[i] = v;
    found[i] = f;
}
// P2, as of an older snapshot: every query has named itself in its slot's owner word (HistIndex::own;
// the word is valid when ids[word] == slot, so nothing of index size is cleared per call); one
// pass over the rows of snapshots 0..s answers for the live row of every wanted slot
__global__ __launch_bounds__(256) void k_hhh_q_scan(const uint4 *log, uint64_t rows, uint32_t s, uint32_t slots,
                                                    const uint32_t *owner, const uint32_t *ids, uint64_t n,
                                                    unsigned long long *values, uint8_t *found) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256) {
        const uint4 q = log[r];
        if (!hhh_live(q, s) || q.x >= slots) continue;
        const uint32_t i = owner[q.x];
        if (i < n && ids[i] == q.x) { values[i] = q.y; found[i] = 1; }
    }
}
// P3: a flow named more than once in the batch takes the answer of the query that owns the slot
__global__ __launch_bounds__(256) void k_hhh_q_dup(const uint32_t *ids, uint64_t n, uint32_t slots, const uint32_t *owner,
                                                   unsigned long long *values, uint8_t *found) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    if (id >= slots) return;
    const uint32_t o = owner[id];
    if (o != (uint32_t)i && o < n) { values[i] = values[o]; found[i] = found[o]; }
}

// Select control words: [0] the value bits fixed so far, [1] rows still wanted at or below the
// band, [2] every row is wanted (fewer than `limit` qualify), [3] rows collected, [4] the cut
enum { SEL_PREFIX = 0, SEL_REM = 1, SEL_ALL = 2, SEL_COUNT = 3, SEL_CUT = 4, SEL_WORDS = 8 };

__global__ void k_hhh_sel_init(uint32_t *ctl, uint32_t limit, uint32_t thr, uint32_t *hist) {
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        ctl[SEL_PREFIX] = 0; ctl[SEL_REM] = limit; ctl[SEL_ALL] = 0; ctl[SEL_COUNT] = 0; ctl[SEL_CUT] = thr;
    }
    for (uint32_t b = t; b < kSelBins; b += blockDim.x) hist[b] = 0;
}

// Q1: one level's histogram of the live rows with value >= thr whose higher bits equal the
// prefix; bin = (value >> shift) & (kSelBins - 1).  `above`: the bits over this level's.
__global__ __launch_bounds__(256) void k_hhh_hist(const uint4 *log, uint64_t rows, uint32_t s, uint32_t thr,
                                                  uint32_t shift, uint32_t above, const uint32_t *ctl, uint32_t *hist) {
    __shared__ uint32_t s_h[kSelBins];
    if (ctl[SEL_ALL]) return;  // (uniform)
    const uint32_t prefix = ctl[SEL_PREFIX];
    for (uint32_t b = threadIdx.x; b < kSelBins; b += 256) s_h[b] = 0;
    __syncthreads();
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256) {
        const uint4 q = log[r];
        if (hhh_live(q, s) && q.y >= thr && ((q.y ^ prefix) & above) == 0)
            atomicAdd(&s_h[(q.y >> shift) & (kSelBins - 1)], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSelBins; b += 256) {
        const uint32_t c = s_h[b];
        if (c) atomicAdd(&hist[b], c);
    }
}
// the band that holds the rem-th largest value; the histogram is cleared for the next level
__global__ __launch_bounds__(256) void k_hhh_pick(uint32_t *hist, uint32_t shift, uint32_t last, uint32_t thr,
                                                  uint32_t *ctl) {
    __shared__ uint32_t s_h[kSelBins];
    for (uint32_t b = threadIdx.x; b < kSelBins; b += 256) {
        s_h[b] = hist[b];
        hist[b] = 0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (!ctl[SEL_ALL]) {
        const uint32_t rem = ctl[SEL_REM];
        uint32_t acc = 0;
        int band = -1;
        for (int b = (int)kSelBins - 1; b >= 0; b--) {
            const uint32_t c = s_h[b];
            if (c >= rem - acc) { band = b; break; }  // acc < rem throughout
            acc += c;
        }
        if (band < 0) {
            ctl[SEL_ALL] = 1;  // fewer than `limit` rows qualify (decided at the first level)
        } else {
            ctl[SEL_PREFIX] |= (uint32_t)band << shift;
            ctl[SEL_REM] = rem - acc;
        }
    }
    if (last) ctl[SEL_CUT] = ctl[SEL_ALL] ? thr : max(thr, ctl[SEL_PREFIX]);
}

// Q2: ballot compaction, one global atomic per workgroup and round.  out: packed rows of
// K + 4 bytes, `cap` of them; rows beyond cap are counted only (the host grows and re-runs).
__global__ __launch_bounds__(256) void k_hhh_collect(const uint4 *log, uint64_t rows, uint32_t s, DictDev D, uint8_t *out,
                                                     uint64_t cap, uint32_t *ctl) {
    __shared__ uint32_t s_w[4], s_base;
    const uint32_t cut = ctl[SEL_CUT], K = D.K, lane = __lane_id(), wv = threadIdx.x >> 6;
    for (uint64_t b0 = (uint64_t)blockIdx.x * 256; b0 < rows; b0 += (uint64_t)gridDim.x * 256) {  // (block-uniform)
        const uint64_t r = b0 + threadIdx.x;
        uint4 q = make_uint4(0, 0, 0, 0);
        bool take = false;
        if (r < rows) {
            q = log[r];
            take = hhh_live(q, s) && q.y >= cut && q.x <= D.mask;
        }
        const uint64_t m = __ballot(take);
        if (lane == 0) s_w[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
            s_base = tot ? atomicAdd(&ctl[SEL_COUNT], tot) : 0u;
        }
        __syncthreads();
        if (take) {
            uint32_t pos = s_base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            for (uint32_t w = 0; w < wv; w++) pos += s_w[w];
            if (pos < cap) {
                const uint32_t *rec = D.rec + (uint64_t)q.x * D.RW + 1;
                uint8_t *o = out + (uint64_t)pos * (K + 4);
                for (uint32_t j = 0; j < K; j++) o[j] = (uint8_t)(rec[j >> 2] >> (8 * (j & 3)));
                o[K] = (uint8_t)q.y; o[K + 1] = (uint8_t)(q.y >> 8); o[K + 2] = (uint8_t)(q.y >> 16); o[K + 3] = (uint8_t)(q.y >> 24);
            }
        }
        __syncthreads();  // s_w / s_base are rewritten by the next round
    }
}

// ordered packed rows -> flows [m, K] and 64-bit values [m] (the host form of a list)
__global__ __launch_bounds__(256) void k_hhh_split(const uint8_t *rows, uint32_t K, uint64_t m, uint8_t *flows,
                                                   unsigned long long *vals) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint8_t *p = rows + i * (uint64_t)(K + 4);
    for (uint32_t j = 0; j < K; j++) flows[i * K + j] = p[j];
    vals[i] = (uint32_t)p[K] | (uint32_t)p[K + 1] << 8 | (uint32_t)p[K + 2] << 16 | (uint32_t)p[K + 3] << 24;
}

// export: log rows [first, first + m) of a lane -> flow bytes, value, writing snapshot
__global__ __launch_bounds__(256) void k_hhh_export(const uint4 *log, uint64_t m, DictDev D, uint8_t *flows,
                                                    uint32_t *vals, uint32_t *written) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint4 q = log[i];
    const uint32_t K = D.K;
    if (q.x <= D.mask) {
        const uint32_t *rec = D.rec + (uint64_t)q.x * D.RW + 1;
        for (uint32_t j = 0; j < K; j++) flows[i * K + j] = (uint8_t)(rec[j >> 2] >> (8 * (j & 3)));
    }
    vals[i] = q.y;
    written[i] = q.z;
}

struct HhLane {
    uint4 *log = nullptr;      // cap rows of room
    uint64_t cap = 0;
    uint32_t *head = nullptr;  // [slots] newest log row of the slot's flow in this lane (kHistOpen: none)
    uint64_t keys = 0;         // flows the lane has listed
};
}  // namespace
}  // namespace gns

using namespace gns;

// The history of one task and one flow width.  Its stream, mutex and pinned staging are its
// own, as a view's: appends and queries from any thread are serialised by the mutex and
// allocate nothing once warm.
struct gns_hh_hist : ViewCore {
    int device = 0;
    uint32_t K = 0;
    uint64_t init_rows = 0;
    HhHistPlan plan;            // timestamps, published rows per lane (host)
    std::vector<HhLane> lanes;  // as plan.lanes
    HistIndex ix;               // the key index (ids: list after list; fresh[0]: pairs the running append added)
    uint64_t pairs = 0;
    uint8_t *stage = nullptr;   // host lists staged for the append
    uint64_t stage_n = 0;
    uint64_t n_log_grow = 0;
    uint32_t *tsc = nullptr;  // a trim's counters, block counts and scan sums
    uint64_t tsc_n = 0;
    // query side
    uint32_t *ctl = nullptr, *hist = nullptr;
    uint8_t *coll = nullptr, *ordered = nullptr;  // collected rows, then in canonical order
    uint64_t coll_n = 0, ordered_n = 0;           // bytes
    uint8_t *spl = nullptr;                       // split / export staging
    uint64_t spl_n = 0;
    HhScratch hh;
    PinnedOut po;
};

namespace {

void hhh_free(gns_hh_hist *h) {
    for (HhLane &l : h->lanes) { dfree(l.log); dfree(l.head); }
    h->lanes.clear();
    h->ix.free_all();
    dfree(h->stage); dfree(h->ctl); dfree(h->hist); dfree(h->coll); dfree(h->ordered); dfree(h->spl); dfree(h->tsc);
    h->hh.free_all();
    h->po.free_all();
    h->destroy();
}

unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }
unsigned scan_grid(uint64_t rows) { return (unsigned)std::min<uint64_t>(2048, (rows + 255) / 256); }

// device rows a caller hands in or takes out lie in device memory of the history's GPU
int hhh_check_dev(const void *p, int device, const char *what) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        set_error("heavy history: %s is not device memory", what);
        return GNS_E_ARG;
    }
    if (a.type != hipMemoryTypeDevice || a.device != device) {
        set_error("heavy history: %s is not memory of device %d", what, device);
        return GNS_E_ARG;
    }
    return GNS_OK;
}

// the lane of `type`, created empty when there is none
int hhh_lane(gns_hh_hist *h, uint32_t type, int *out) {
    int l = h->plan.lane(type);
    if (l < 0) {
        HhLane ln;
        GNS_TRY(dalloc_t(&ln.head, h->ix.slots));
        if (hipMemsetAsync(ln.head, 0xFF, h->ix.slots * 4, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
            dfree(ln.head);
            set_error("heavy history: lane clear failed");
            return GNS_E_HIP;
        }
        l = h->plan.add_lane(type);
        h->lanes.push_back(ln);
    }
    *out = l;
    return GNS_OK;
}

// Room for `need` rows in lane l: allocate, copy the published rows, free (before anything is linked).
int hhh_reserve_log(gns_hh_hist *h, int l, uint64_t need) {
    HhLane &ln = h->lanes[(size_t)l];
    if (need <= ln.cap) return GNS_OK;
    const uint64_t cap = hist_row_capacity(ln.cap ? ln.cap : std::min<uint64_t>(h->init_rows, kHistMax), need);
    const uint64_t rows = h->plan.lanes[(size_t)l].rows;
    uint4 *g = nullptr;
    GNS_TRY(dalloc_t(&g, cap));
    if (rows) {
        hipError_t e = hipMemcpyAsync(g, ln.log, rows * sizeof(uint4), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            dfree(g);
            set_error("heavy history log growth: %s", hipGetErrorString(e));
            return GNS_E_HIP;
        }
    }
    if (ln.cap) h->n_log_grow++;
    dfree(ln.log);
    ln.log = g;
    ln.cap = cap;
    return GNS_OK;
}

// HistIndex::resolve's growth: every lane's head words follow the records, and so does the slot
// column of its log.  m != 0: room for a piece of m flows if every one of them is new.
int hhh_grow(gns_hh_hist *h, uint64_t m, uint64_t done) {
    std::vector<uint32_t **> heads;
    for (HhLane &ln : h->lanes) heads.push_back(&ln.head);
    hipStream_t s = h->stream;
    return h->ix.grow(m ? h->ix.room_for(h->ix.claimed + m) : 0, done, heads, s, [&](const uint32_t *remap, uint64_t old_slots) {
        for (size_t i = 0; i < h->lanes.size(); i++) {
            const uint64_t rows = h->plan.lanes[i].rows;
            if (rows) hipLaunchKernelGGL(k_hhh_reslot, dim3(grid256(rows)), dim3(256), 0, s, h->lanes[i].log, rows, old_slots, remap);
        }
    });
}

// Q1-Q3 under h->mu: the list of `type` as of *end_ns in h->ordered, *n rows of it (after the
// cut to `limit`).  Synchronizes the stream.
int hhh_list(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, uint64_t threshold, uint64_t limit, uint64_t *n) {
    *n = 0;
    const int64_t sn = h->plan.t.as_of(end_ns);
    const int l = h->plan.lane(type);
    const uint64_t rows = h->plan.rows_as_of(l, sn);
    if (rows == 0 || threshold > 0xFFFFFFFFull) return GNS_OK;  // (values are 32-bit)
    hipStream_t st = h->stream;
    const HhLane &ln = h->lanes[(size_t)l];
    const uint32_t s = (uint32_t)sn, thr = (uint32_t)threshold, K = h->K;
    const uint32_t lim = (uint32_t)std::min<uint64_t>(limit, 0xFFFFFFFFull);  // (a lane holds fewer rows)
    const dim3 grid(scan_grid(rows));
    hipLaunchKernelGGL(k_hhh_sel_init, dim3(1), dim3(256), 0, st, h->ctl, lim, thr, h->hist);
    if (lim) {
        const uint32_t shift[3] = {21, 10, 0}, above[3] = {0u, 0xFFE00000u, 0xFFFFFC00u};
        for (int lv = 0; lv < 3; lv++) {
            hipLaunchKernelGGL(k_hhh_hist, grid, dim3(256), 0, st, ln.log, rows, s, thr, shift[lv], above[lv], h->ctl, h->hist);
            hipLaunchKernelGGL(k_hhh_pick, dim3(1), dim3(256), 0, st, h->hist, shift[lv], lv == 2 ? 1u : 0u, thr, h->ctl);
        }
    }
    GNS_HIP(hipGetLastError());
    uint32_t *hp = reinterpret_cast<uint32_t *>(h->po.pin);
    uint64_t got = 0;
    for (int pass = 0; pass < 2; pass++) {
        const uint64_t cap = h->coll ? h->coll_n / (K + 4) : 0;
        hipLaunchKernelGGL(k_hhh_collect, grid, dim3(256), 0, st, ln.log, rows, s, h->ix.D, h->coll, cap, h->ctl);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipMemcpyAsync(hp, h->ctl + SEL_COUNT, 4, hipMemcpyDeviceToHost, st));
        GNS_HIP(hipStreamSynchronize(st));
        got = *hp;
        if (got <= cap) break;
        // more rows than the buffer holds: grow to the count and collect again (the cut stands)
        GNS_TRY(grow_buf(&h->coll, h->coll_n, got * (K + 4)));
        GNS_HIP(hipMemsetAsync(h->ctl + SEL_COUNT, 0, 4, st));
    }
    if (got == 0) return GNS_OK;
    if (got >= (1ull << 31)) { set_error("heavy history: a list of %llu rows (max 2^31 - 1)", (unsigned long long)got); return GNS_E_RANGE; }
    GNS_TRY(grow_buf(&h->ordered, h->ordered_n, got * (K + 4)));
    GNS_TRY(hh_order_rows_dev(h->hh, st, h->coll, K, (uint32_t)got, h->ordered));
    GNS_HIP(hipStreamSynchronize(st));
    *n = limit ? std::min<uint64_t>(got, limit) : got;
    return GNS_OK;
}

// T2 on the host side: a[0, n) -> its exclusive scan, the total to *tot.  sc: room for the tile
// sums of every level below, hhh_scan_words(n) words.
uint64_t hhh_scan_words(uint64_t n) {
    uint64_t w = 0;
    while (n > kScanTile) {
        n = (n + kScanTile - 1) / kScanTile;
        w += n;
    }
    return w;
}
void hhh_scan(hipStream_t s, uint32_t *a, uint64_t n, uint32_t *sc, uint32_t *tot) {
    if (n <= kScanTile) {
        hipLaunchKernelGGL(k_hhh_scan, dim3(1), dim3(256), 0, s, a, n, tot);
        return;
    }
    const uint64_t nt = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_hhh_scan, dim3((unsigned)nt), dim3(256), 0, s, a, n, sc);
    hhh_scan(s, sc, nt, sc + nt, tot);
    hipLaunchKernelGGL(k_hhh_scan_add, dim3(grid256(n)), dim3(256), 0, s, a, n, (const uint32_t *)sc);
}

}  // namespace

extern "C" {

int gns_hh_hist_create(const gns_hh_hist_params *p, gns_hh_hist **out) {
    if (!p || !out) { set_error("null argument"); return GNS_E_ARG; }
    *out = nullptr;
    if (p->key_bytes == 0 || p->key_bytes > 37) { set_error("heavy history: key_bytes %u (1..37)", p->key_bytes); return GNS_E_ARG; }
    if (p->max_rows > kHistMax || p->max_flows > kDictMaxSlots / 2) { set_error("heavy history capacity too large"); return GNS_E_ARG; }
    GNS_TRY(check_device(p->device));
    gns_hh_hist *h = new gns_hh_hist();
    h->device = p->device;
    h->K = p->key_bytes;
    h->init_rows = p->max_rows ? p->max_rows : (1ull << 20);
    int rc = GNS_OK;
    do {
        if ((rc = set_device(h->device)) != GNS_OK) break;
        if ((rc = h->init()) != GNS_OK || (rc = h->po.reserve(0)) != GNS_OK) break;
        if ((rc = dalloc_t(&h->ctl, SEL_WORDS)) || (rc = dalloc_t(&h->hist, kSelBins))) break;
        rc = h->ix.init("heavy history", h->K, hist_index_slots(p->max_flows ? p->max_flows : (64ull << 10)), h->stream);
    } while (0);
    if (rc != GNS_OK) { hhh_free(h); delete h; return rc; }
    *out = h;
    return GNS_OK;
}

int gns_hh_hist_destroy(gns_hh_hist *h) {
    if (!h) return GNS_OK;
    (void)hipSetDevice(h->device);
    h->quiesce();
    hhh_free(h);
    delete h;
    return GNS_OK;
}

int gns_hh_hist_append(gns_hh_hist *h, int64_t timestamp_ns, const gns_hh_list *lists, uint32_t nlists, gns_mem where,
                       uint64_t out[2]) {
    if (!h || (nlists && !lists)) { set_error("null argument"); return GNS_E_ARG; }
    if (nlists > kHhTypes) { set_error("heavy history append: %u lists (at most one per type)", nlists); return GNS_E_ARG; }
    if (where != GNS_MEM_HOST && where != GNS_MEM_DEVICE) { set_error("heavy history append: unknown memory kind"); return GNS_E_ARG; }
    uint32_t types[kHhTypes];
    uint64_t ns[kHhTypes], total = 0;
    for (uint32_t i = 0; i < nlists; i++) {
        if (lists[i].n && !lists[i].rows) { set_error("null argument"); return GNS_E_ARG; }
        types[i] = lists[i].type;
        ns[i] = lists[i].n;
        total += lists[i].n;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    const int chk = h->plan.append_check(timestamp_ns, types, ns, nlists);
    switch (chk) {
    case HIST_OK: break;
    case HIST_E_TIME:
        set_error("heavy history append: timestamp %lld is not after the last snapshot's %lld", (long long)timestamp_ns,
                  (long long)h->plan.t.ts.back());
        return GNS_E_ARG;
    case HIST_E_SNAPSHOTS: set_error("heavy history holds 2^32 - 2 snapshots"); return GNS_E_FULL;
    case HIST_E_ROWS: set_error("heavy history: a type's log cannot grow beyond 2^32 - 2 rows"); return GNS_E_FULL;
    case HHH_E_TYPE: set_error("heavy history append: a list's type is outside 0..255"); return GNS_E_ARG;
    default: set_error("heavy history append: two lists of one type"); return GNS_E_ARG;
    }
    GNS_TRY(set_device(h->device));
    hipStream_t s = h->stream;
    const uint32_t W = h->K + 4, S = (uint32_t)h->plan.t.ts.size();
    if (where == GNS_MEM_DEVICE)
        for (uint32_t i = 0; i < nlists; i++)
            if (lists[i].n) GNS_TRY(hhh_check_dev(lists[i].rows, h->device, "a list's rows"));
    uint64_t fresh = 0;
    if (total) {
        // room first: lanes, their logs, the ids, and device copies of host lists
        int lane[kHhTypes];
        for (uint32_t i = 0; i < nlists; i++) {
            if (ns[i] == 0) { lane[i] = -1; continue; }
            GNS_TRY(hhh_lane(h, types[i], &lane[i]));
            GNS_TRY(hhh_reserve_log(h, lane[i], h->plan.lanes[(size_t)lane[i]].rows + ns[i]));
        }
        HistIndex &ix = h->ix;
        if (ix.ids_n < total) GNS_TRY(grow_buf(&ix.ids, ix.ids_n, total));
        const uint8_t *rows[kHhTypes];
        if (where == GNS_MEM_HOST) {
            if (h->stage_n < total * W) GNS_TRY(grow_buf(&h->stage, h->stage_n, total * W));
            uint64_t at = 0;
            for (uint32_t i = 0; i < nlists; i++) {
                rows[i] = h->stage + at * W;
                if (ns[i]) GNS_TRY(h->po.copy_in(h->stage + at * W, lists[i].rows, ns[i] * W, s));
                at += ns[i];
            }
        } else {
            for (uint32_t i = 0; i < nlists; i++) rows[i] = lists[i].rows;
        }
        // A1: every list, before anything is checked or linked (a growth renumbers the ids)
        uint64_t at = 0;
        for (uint32_t i = 0; i < nlists; i++) {
            GNS_TRY(ix.resolve(rows[i], W, ns[i], at, s, [&](uint64_t m, uint64_t done) { return hhh_grow(h, m, done); }));
            at += ns[i];
        }
        // A1b: no two rows of a list in one index slot
        uint32_t *hp = reinterpret_cast<uint32_t *>(h->po.pin);
        GNS_HIP(hipMemsetAsync(ix.fresh, 0, 8, s));
        at = 0;
        for (uint32_t i = 0; i < nlists; i++) {
            if (ns[i]) GNS_TRY(ix.check_unique(ix.ids + at, ns[i], ix.fresh + 1, s));
            at += ns[i];
        }
        GNS_HIP(hipMemcpyAsync(hp, ix.fresh + 1, 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));
        if (*hp) { set_error("heavy history append: two rows of a list name the same flow"); return GNS_E_ARG; }
        // A2
        at = 0;
        uint64_t added[kHhTypes] = {};
        for (uint32_t i = 0; i < nlists; i++) {
            if (ns[i] == 0) continue;
            HhLane &ln = h->lanes[(size_t)lane[i]];
            GNS_HIP(hipMemsetAsync(ix.fresh, 0, 4, s));
            hipLaunchKernelGGL(k_hhh_link, dim3(grid256(ns[i])), dim3(256), 0, s, rows[i], h->K, ns[i], ix.ids + at, ln.head,
                               (uint32_t)ix.slots, ln.log, ln.cap, h->plan.lanes[(size_t)lane[i]].rows, S, ix.fresh);
            GNS_HIP(hipGetLastError());
            GNS_HIP(hipMemcpyAsync(hp + 1 + i, ix.fresh, 4, hipMemcpyDeviceToHost, s));
            at += ns[i];
        }
        GNS_HIP(hipStreamSynchronize(s));  // the caller's rows are read
        for (uint32_t i = 0; i < nlists; i++) {
            if (ns[i] == 0) continue;
            added[i] = hp[1 + i];
            h->lanes[(size_t)lane[i]].keys += added[i];
            fresh += added[i];
        }
    }
    h->pairs += fresh;
    // (a list without rows names no lane: publish only what has one)
    uint32_t pt[kHhTypes];
    uint64_t pn[kHhTypes];
    uint32_t np = 0;
    for (uint32_t i = 0; i < nlists; i++)
        if (ns[i]) { pt[np] = types[i]; pn[np] = ns[i]; np++; }
    h->plan.publish(timestamp_ns, pt, pn, np);  // last: the snapshot exists from here on
    if (out) { out[0] = total; out[1] = fresh; }
    return GNS_OK;
}

int gns_hh_hist_heavy_rows(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, uint64_t threshold, uint64_t limit,
                           uint8_t *rows_dev, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    if (rows_dev && *n_io) GNS_TRY(hhh_check_dev(rows_dev, h->device, "rows_dev"));
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t cap = *n_io;
    uint64_t n = 0;
    GNS_TRY(hhh_list(h, end_ns, type, threshold, limit, &n));
    *n_io = n;
    if (n == 0 || n > cap || !rows_dev) return GNS_OK;
    GNS_HIP(hipMemcpyAsync(rows_dev, h->ordered, n * (h->K + 4), hipMemcpyDeviceToDevice, h->stream));
    GNS_HIP(hipStreamSynchronize(h->stream));
    return GNS_OK;
}

int gns_hh_hist_heavy_hitters(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, uint64_t threshold, uint64_t limit,
                              uint8_t *flows, uint64_t *values, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t cap = *n_io;
    uint64_t n = 0;
    GNS_TRY(hhh_list(h, end_ns, type, threshold, limit, &n));
    *n_io = n;
    if (n == 0 || n > cap || !(flows || values)) return GNS_OK;
    hipStream_t s = h->stream;
    const uint32_t K = h->K;
    if (h->spl_n < n * (K + 8)) GNS_TRY(grow_buf(&h->spl, h->spl_n, n * (K + 8)));
    unsigned long long *dv = reinterpret_cast<unsigned long long *>(h->spl);
    uint8_t *df = h->spl + n * 8;
    hipLaunchKernelGGL(k_hhh_split, dim3(grid256(n)), dim3(256), 0, s, h->ordered, K, n, df, dv);
    GNS_HIP(hipGetLastError());
    if (flows) GNS_TRY(h->po.copy_out(flows, df, n * K, s));
    if (values) GNS_TRY(h->po.copy_out(values, dv, n * 8, s));
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

int gns_hh_hist_times(gns_hh_hist *h, int64_t *ts, uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t n = h->plan.t.ts.size(), m = std::min<uint64_t>(*n_io, n);
    *n_io = n;
    if (ts)
        for (uint64_t i = 0; i < m; i++) ts[i] = h->plan.t.ts[(size_t)i];
    return GNS_OK;
}

int gns_hh_hist_stats(gns_hh_hist *h, uint64_t out[8]) {
    if (!h || !out) { set_error("null argument"); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    uint64_t cap = 0;
    for (const HhLane &l : h->lanes) cap += l.cap;
    out[0] = h->plan.t.ts.size(); out[1] = h->plan.t.rows; out[2] = h->pairs; out[3] = h->lanes.size();
    out[4] = cap; out[5] = h->ix.slots; out[6] = h->ix.n_index_grow; out[7] = h->n_log_grow;
    return GNS_OK;
}

int gns_hh_hist_export(gns_hh_hist *h, uint8_t *types, uint8_t *flows, uint32_t *values, uint32_t *written,
                       uint64_t *n_io) {
    if (!h || !n_io) { set_error("null argument"); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t rows = h->plan.t.rows, room = std::min<uint64_t>(*n_io, rows);
    *n_io = rows;
    if (room == 0 || !(types || flows || values || written)) return GNS_OK;
    hipStream_t s = h->stream;
    const uint32_t K = h->K;
    uint64_t at = 0;
    for (uint32_t type = 0; type < kHhTypes && at < room; type++) {  // (type, log order)
        const int l = h->plan.lane(type);
        if (l < 0) continue;
        const uint64_t m = std::min<uint64_t>(h->plan.lanes[(size_t)l].rows, room - at);
        if (m == 0) continue;
        if (types) memset(types + at, (int)type, m);
        if (flows || values || written) {
            if (h->spl_n < m * (K + 8)) GNS_TRY(grow_buf(&h->spl, h->spl_n, m * (K + 8)));
            uint32_t *dv = reinterpret_cast<uint32_t *>(h->spl), *dw = dv + m;
            uint8_t *df = h->spl + m * 8;
            hipLaunchKernelGGL(k_hhh_export, dim3(grid256(m)), dim3(256), 0, s, h->lanes[(size_t)l].log, m, h->ix.D, df, dv, dw);
            GNS_HIP(hipGetLastError());
            if (flows) GNS_TRY(h->po.copy_out(flows + at * K, df, m * K, s));
            if (values) GNS_TRY(h->po.copy_out(values + at, dv, m * 4, s));
            if (written) GNS_TRY(h->po.copy_out(written + at, dw, m * 4, s));
            GNS_HIP(hipStreamSynchronize(s));
        }
        at += m;
    }
    return GNS_OK;
}

int gns_hh_hist_trim(gns_hh_hist *h, int64_t before_ns, int fold, uint64_t out[4]) {
    if (!h) { set_error("null argument"); return GNS_E_ARG; }
    if (fold != 0 && fold != 1) { set_error("heavy history trim: fold %d (0: drop, 1: fold)", fold); return GNS_E_ARG; }
    std::lock_guard<std::mutex> lk(h->mu);
    const HhHistPlan::Trim tp = h->plan.trim_plan(before_ns, fold != 0);
    if (out) { out[0] = out[1] = out[2] = 0; out[3] = h->plan.t.rows; }
    if (tp.t.noop) return GNS_OK;
    GNS_TRY(set_device(h->device));
    hipStream_t s = h->stream;
    const size_t nl = h->lanes.size();
    HistIndex &ix = h->ix;
    const uint64_t old_slots = ix.slots;
    const uint32_t s_last = (uint32_t)(tp.t.c - 1), d = tp.t.d;
    // scratch: [0, nl) rows each lane's base keeps, [nl, 2 nl) pairs each lane forgets, [2 nl] keys
    // still named; then per ranked lane its block counts and the scan's tile sums
    std::vector<uint64_t> at(nl, 0), nblk(nl, 0), nbase(nl, 0);
    uint64_t words = 2 * nl + 1;
    bool ranked = false;
    for (size_t l = 0; l < nl; l++) {
        if (!tp.t.fold || tp.R[l] == 0) continue;  // prefix rows may stay
        nblk[l] = (tp.R[l] + 255) / 256;
        at[l] = words;
        words += nblk[l] + hhh_scan_words(nblk[l]);
        ranked = true;
    }
    if (h->tsc_n < words) GNS_TRY(grow_buf(&h->tsc, h->tsc_n, words));
    uint32_t *hp = reinterpret_cast<uint32_t *>(h->po.pin);
    GNS_HIP(hipMemsetAsync(h->tsc, 0, (2 * nl + 1) * 4, s));
    if (ranked) {  // T1 / T2 as of the last expired snapshot
        for (size_t l = 0; l < nl; l++) {
            if (!nblk[l]) continue;
            uint32_t *cnt = h->tsc + at[l];
            hipLaunchKernelGGL(k_hhh_trim_count, dim3((unsigned)nblk[l]), dim3(256), 0, s, (const uint4 *)h->lanes[l].log,
                               tp.R[l], s_last, cnt);
            hhh_scan(s, cnt, nblk[l], cnt + nblk[l], h->tsc + l);
        }
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipMemcpyAsync(hp, h->tsc, nl * 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));
        for (size_t l = 0; l < nl; l++) nbase[l] = hp[l];
    }
    // everything new is built beside the history, which stays as it is until the end
    std::vector<HhLane> nw(nl);
    std::vector<uint32_t *> nh(nl, nullptr);  // the head words at the rebuilt index's slots
    std::vector<uint64_t> forgot(nl, 0);
    uint64_t forgot_all = 0;
    auto run = [&]() -> int {
        const dim3 sgrid(grid256(old_slots));
        for (size_t l = 0; l < nl; l++) {
            const uint64_t rows = h->plan.lanes[l].rows, kept = rows - tp.R[l] + nbase[l];
            GNS_TRY(dalloc_t(&nw[l].head, old_slots));
            GNS_HIP(hipMemsetAsync(nw[l].head, 0xFF, old_slots * 4, s));
            if (kept) {
                nw[l].cap = hist_row_capacity(0, kept);
                GNS_TRY(dalloc_t(&nw[l].log, nw[l].cap));
                HhTrim t{};
                t.rows = rows; t.R = tp.R[l]; t.nbase = nbase[l]; t.row0 = nblk[l] ? 0 : tp.R[l]; t.cap = nw[l].cap;
                t.s_last = s_last; t.d = d; t.fold = tp.t.fold ? 1 : 0;
                hipLaunchKernelGGL(k_hhh_trim_move, dim3(grid256(rows - t.row0)), dim3(256), 0, s, (const uint4 *)h->lanes[l].log,
                                   t, (const uint32_t *)(nblk[l] ? h->tsc + at[l] : nullptr), nw[l].log);
                hipLaunchKernelGGL(k_hhh_trim_heads, dim3(grid256(kept)), dim3(256), 0, s, (const uint4 *)nw[l].log, kept,
                                   old_slots, nw[l].head);
            }
            hipLaunchKernelGGL(k_hhh_trim_forgot, sgrid, dim3(256), 0, s, (const uint32_t *)h->lanes[l].head,
                               (const uint32_t *)nw[l].head, old_slots, h->tsc + nl + l);
            GNS_HIP(hipGetLastError());
        }
        std::vector<const uint32_t *> heads;
        for (const HhLane &ln : nw) heads.push_back(ln.head);
        GNS_TRY(ix.mark_heads(heads.data(), nl, s));
        hipLaunchKernelGGL(k_hhh_trim_named, sgrid, dim3(256), 0, s, (const uint32_t *)ix.mark, old_slots, h->tsc + 2 * nl);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipMemcpyAsync(hp, h->tsc + nl, (nl + 1) * 4, hipMemcpyDeviceToHost, s));
        GNS_HIP(hipStreamSynchronize(s));
        for (size_t l = 0; l < nl; l++) {
            forgot[l] = hp[l];
            forgot_all += forgot[l];
        }
        if (!forgot_all) return GNS_OK;
        // the index rebuilt from the keys some lane still names, into a table of their number
        // (never a larger one: the named keys fit the table they are in)
        const uint64_t want = std::min<uint64_t>(hist_index_slots(hp[nl]), old_slots);
        for (size_t l = 0; l < nl; l++) {
            GNS_TRY(dalloc_t(&nh[l], want));
            GNS_HIP(hipMemsetAsync(nh[l], 0xFF, want * 4, s));
        }
        GNS_TRY(ix.shrink_beside(want, s));
        for (size_t l = 0; l < nl; l++) {
            const uint64_t kept = h->plan.lanes[l].rows - tp.R[l] + nbase[l];
            ix.permute(nw[l].head, old_slots, nh[l], s);
            if (kept) hipLaunchKernelGGL(k_hhh_reslot, dim3(grid256(kept)), dim3(256), 0, s, nw[l].log, kept, old_slots,
                                         (const uint32_t *)ix.dsc.remap);
        }
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipStreamSynchronize(s));
        return GNS_OK;
    };
    const int rc = run();
    if (rc != GNS_OK) {
        (void)hipStreamSynchronize(s);
        ix.rollback();
        for (size_t l = 0; l < nl; l++) { dfree(nw[l].log); dfree(nw[l].head); dfree(nh[l]); }
        return rc;
    }
    // publish: the logs, the index and the head words, then the plan
    uint64_t removed = 0;
    for (size_t l = 0; l < nl; l++) {
        HhLane &ln = h->lanes[l];
        dfree(ln.log);
        dfree(ln.head);
        ln.log = nw[l].log;
        ln.cap = nw[l].cap;
        if (nh[l]) { dfree(nw[l].head); ln.head = nh[l]; }  // (the index was rebuilt)
        else ln.head = nw[l].head;
        ln.keys -= forgot[l];
        removed += tp.R[l] - nbase[l];
    }
    ix.commit();
    h->pairs -= forgot_all;
    h->plan = h->plan.trimmed(tp, nbase);
    if (out) { out[0] = tp.t.fold ? tp.t.c - 1 : tp.t.c; out[1] = removed; out[2] = forgot_all; out[3] = h->plan.t.rows; }
    return GNS_OK;
}

int gns_hh_hist_query(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, const uint8_t *flows, uint64_t n, gns_mem where,
                      uint64_t *values, uint8_t *found) {
    if (!h || (n && !(flows && values && found))) { set_error("null argument"); return GNS_E_ARG; }
    if (where != GNS_MEM_HOST && where != GNS_MEM_DEVICE) { set_error("heavy history query: unknown memory kind"); return GNS_E_ARG; }
    if (n == 0) return GNS_OK;
    if (n > kHistMax) { set_error("heavy history query: %llu flows in one call", (unsigned long long)n); return GNS_E_ARG; }
    GNS_TRY(set_device(h->device));
    const bool dev = where == GNS_MEM_DEVICE;
    if (dev) {
        GNS_TRY(hhh_check_dev(flows, h->device, "flows"));
        GNS_TRY(hhh_check_dev(values, h->device, "values"));
        GNS_TRY(hhh_check_dev(found, h->device, "found"));
    }
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t s = h->stream;
    const uint32_t K = h->K;
    const int64_t sn = h->plan.t.as_of(end_ns);
    const int l = h->plan.lane(type);
    const uint64_t rows = h->plan.rows_as_of(l, sn);
    if (rows == 0) {  // no row of this type by then: nothing is live
        if (dev) {
            GNS_HIP(hipMemsetAsync(values, 0, n * 8, s));
            GNS_HIP(hipMemsetAsync(found, 0, n, s));
            GNS_HIP(hipStreamSynchronize(s));
        } else {
            memset(values, 0, n * 8);
            memset(found, 0, n);
        }
        return GNS_OK;
    }
    const uint8_t *df = flows;
    unsigned long long *dv = reinterpret_cast<unsigned long long *>(values);
    uint8_t *dfound = found;
    if (!dev) {  // keys in, answers out through the history's own buffers
        if (h->stage_n < n * K) GNS_TRY(grow_buf(&h->stage, h->stage_n, n * K));
        if (h->spl_n < n * 9) GNS_TRY(grow_buf(&h->spl, h->spl_n, n * 9));
        GNS_TRY(h->po.copy_in(h->stage, flows, n * K, s));
        df = h->stage;
        dv = reinterpret_cast<unsigned long long *>(h->spl);
        dfound = h->spl + n * 8;
    }
    HistIndex &ix = h->ix;
    if (ix.ids_n < n) GNS_TRY(grow_buf(&ix.ids, ix.ids_n, n));
    const HhLane &ln = h->lanes[(size_t)l];
    const bool newest = sn == (int64_t)h->plan.t.ts.size() - 1;
    const dim3 qgrid(grid256(n));
    hipLaunchKernelGGL(k_hhh_q_lookup, qgrid, dim3(256), 0, s, df, n, ix.D, (const uint32_t *)(newest ? ln.head : nullptr),
                       (const uint4 *)ln.log, rows, ix.ids, dv, dfound);
    if (!newest) {
        GNS_TRY(ix.own(ix.ids, n, s));
        hipLaunchKernelGGL(k_hhh_q_scan, dim3(scan_grid(rows)), dim3(256), 0, s, (const uint4 *)ln.log, rows, (uint32_t)sn,
                           (uint32_t)ix.slots, (const uint32_t *)ix.mark, (const uint32_t *)ix.ids, n, dv, dfound);
        hipLaunchKernelGGL(k_hhh_q_dup, qgrid, dim3(256), 0, s, (const uint32_t *)ix.ids, n, (uint32_t)ix.slots,
                           (const uint32_t *)ix.mark, dv, dfound);
    }
    GNS_HIP(hipGetLastError());
    if (!dev) {
        GNS_TRY(h->po.copy_out(values, dv, n * 8, s));
        GNS_TRY(h->po.copy_out(found, dfound, n, s));
    }
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

}  // extern "C"
