// gns_common.hpp -- host-side plumbing shared by the engines: error reporting,
// the device check and set, device buffers, per-stage HIP-event timing, advancing
// and staging of host inputs into device memory, and the flow dictionary's
// ownership, reclaim and batch recovery, and its key resolution for the imports;
// and the read side: pinned copy-out, the point-query call and a view's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gns_sketch.h"
#include "gns_device.cuh"
#include "gns_keys.cuh"
#include "gns_pinchunk.hpp"

namespace gns {

void set_error(const char *fmt, ...);

#define GNS_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            ::gns::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call,                \
                             hipGetErrorString(e_));                                   \
            return GNS_E_HIP;                                                          \
        }                                                                              \
    } while (0)

#define GNS_TRY(expr)                  \
    do {                               \
        int r_ = (expr);               \
        if (r_ != GNS_OK) return r_;   \
    } while (0)

// Device allocation that reports OOM as GNS_E_OOM.
int dalloc(void **p, size_t bytes);
template <class T>
int dalloc_t(T **p, size_t count) {
    return dalloc(reinterpret_cast<void **>(p), count * sizeof(T) + 16);
}
void dfree(void *p);
// Grow-only buffer, to twice the request: heavy-hitter lists grow window by
// window over a period, and every reallocation (hipFree synchronizes the device)
// cost more than the whole device-side list build.
template <typename T>
int grow_buf(T **p, uint64_t &have, uint64_t need) {
    if (need <= have && *p) return GNS_OK;
    dfree(*p);
    *p = nullptr;
    have = 0;
    const uint64_t n = std::max<uint64_t>(2 * need, 1);
    GNS_TRY(dalloc(reinterpret_cast<void **>(p), n * sizeof(T)));
    have = n;
    return GNS_OK;
}

// A device exists and `device` names one (GNS_E_NODEV / GNS_E_ARG).
int check_device(int device);
// Clears a stale error of an earlier runtime call on this thread (e.g. the host
// framework's: it must not fail this call's launch checks) and sets the device.
int set_device(int device);

// Stream `waiter` waits for what is queued on stream `on` now: one handle's kernels reading
// another's state at this point of its stream.  GNS_E_HIP with "<what>: <runtime's text>".
int stream_wait_now(hipStream_t waiter, hipStream_t on, const char *what);

// Test-only piece size of a roll-up (GNS_EX_ROLLUP_PIECE, GNS_SPREAD_ROLLUP_PIECE: small
// tables span many pieces): the variable's value when it is set, nonzero and below dflt.
uint64_t test_piece(const char *env_name, uint64_t dflt);

// `in` from record `off` on: every per-record array that is set.
InputDesc advance(const InputDesc &in, uint64_t off);

// Host batches staged into one grow-only device buffer: each item's bytes are
// copied on the stream, one after the other at 16-byte boundaries, and *patch is
// pointed at the copy.  An item without bytes is skipped; one without a source
// only gets its room (the engine fills it on the stream).
struct StageItem {
    const void *src;
    size_t bytes;
    const void **patch;
};
using StageList = std::vector<StageItem>;
template <class T>
void stage_add(StageList &l, const T *src, size_t bytes, const T **patch) {
    l.push_back({src, bytes, reinterpret_cast<const void **>(patch)});
}
// the first m records of host batch d: every per-record array that is set is to
// be staged (hdr, tuple arrays, keys, keys2, rec16, then sizes) and d pointed at it
void stage_input(StageList &l, InputDesc &d, uint64_t m);
struct HostStage {
    uint8_t *buf = nullptr;
    size_t cap = 0;
    static size_t need(const StageList &l);
    int copy(const StageList &l, hipStream_t s);  // grows the buffer to need(l) first
    void free_all();
};

// What an engine keeps for compact records (IN_REC16; gns_records.hip): the side
// records of a host call, staged once (escapes index the side array of the whole
// call, so it is never advanced with the batches), and the size array of a batch of
// the 16-byte form (the escapes' parse and the engines read sizes[p]).
struct CompactInput {
    uint32_t *side_dev = nullptr;
    uint64_t side_n = 0;
    uint32_t *sizes = nullptr;
    uint64_t sizes_n = 0;
    // in.side -> a device copy of the host side array.  Waits for stream s first:
    // the batches of the previous call may still read the buffer.
    int stage_side(InputDesc &in, hipStream_t s);
    // 16-byte form: the wire lengths of d's first m records (device memory) unpacked
    // on stream s, d.sizes pointed at them.  The 20-byte form is left as it is.
    // (reserve: room for at least that many records, so that later batches do not reallocate)
    int unpack_sizes(InputDesc &d, uint64_t m, hipStream_t s, uint64_t reserve = 0);
    // the same into room the caller owns (a staged batch's)
    static int unpack_sizes_into(const uint32_t *rec16, uint64_t m, uint32_t *dst, hipStream_t s);
    void free_all();
};
// The descriptor of a gns_*_insert_compact call (wirelen == NULL: the 16-byte form).
InputDesc compact_desc(const uint8_t *rec16, const uint32_t *wirelen, const uint8_t *side64, uint64_t n_side);
// ... of a gns_*_insert_tuples call (the null checks are the engine's) and of gns_*_insert_headers
inline InputDesc tuples_desc(const gns_tuples &t, bool with_length) {
    InputDesc in{};
    in.src16 = t.src16; in.dst16 = t.dst16; in.sport = t.sport; in.dport = t.dport; in.proto = t.proto;
    in.sizes = with_length ? t.length : nullptr;
    return in;
}
inline InputDesc headers_desc(const uint8_t *hdr, const uint32_t *wirelen) {
    InputDesc in{};
    in.hdr = reinterpret_cast<const uint32_t *>(hdr);
    in.sizes = wirelen;
    return in;
}

// Flow-key plan from a configured layout (task.go:265-300, :327-338).
int make_plan(const gns_layout &l, uint32_t key_bytes, KeyPlanN *out);
// plan for the concatenation a ‖ b (SuperSpread merged key, super_spread.go:183-190)
int make_plan2(const gns_layout &a, const gns_layout &b, KeyPlanN *out);
uint32_t layout_bytes(const gns_layout &l);

// Per-stage timing with HIP events recorded on the engine stream.
struct StageTimer {
    enum { kStages = 8 };
    bool on = false;
    uint32_t mask = 0xFFFFFFFFu;  // stages timed while on
    double ms[kStages] = {};
    uint64_t launches[kStages] = {};
    std::vector<hipEvent_t> pool;
    struct Pending { hipEvent_t a, b; int stage; };
    std::vector<Pending> pending;
    hipStream_t stream = nullptr;

    hipEvent_t get();
    void begin(int stage, hipEvent_t *a);
    void end(int stage, hipEvent_t a);
    int collect();  // synchronizes pending events and accumulates
    // gns_*_stage_times: collects, copies the totals out (either may be null), clears them on reset
    void report(double *ms_out, uint64_t *launches_out, int reset);
    void destroy();
};
// gns_*_flush: everything queued on the handle's stream has run, its stage times are collected
int handle_flush(int device, hipStream_t stream, StageTimer &timer);

// gns_*_set_timing's argument: 0 off, GNS_TIMING_MASK | stage bits = only those stages (fewer
// events inside a batch), any other nonzero value = every stage
inline void set_timing_arg(StageTimer &t, int on) {
    t.on = on != 0;
    t.mask = (on & GNS_TIMING_MASK) ? ((uint32_t)on & 0xFFu) : 0xFFFFFFFFu;
}

struct ScopedStage {
    StageTimer &t; int stage; hipEvent_t a = nullptr;
    ScopedStage(StageTimer &tt, int s) : t(tt), stage(s) { t.begin(stage, &a); }
    ~ScopedStage() { t.end(stage, a); }
};

// splitmix64 row seeds used when the caller passes none.
void default_seeds(uint32_t *out, uint32_t n);

// Dictionary record words {tag, key words}: a power of two (4, 8 or 16 words)
// so that no record straddles a 64-byte line (one line per probe).
inline uint32_t dict_record_words(uint32_t K) {
    const uint32_t w = 1 + (K + 3) / 4;
#ifdef GNS_DICT_PACKED
    return (w + 3) & ~3u;
#else
    return w <= 4 ? 4u : (w <= 8 ? 8u : 16u);
#endif
}

// Count-Min records: 16 words whenever the key leaves words 12..15 free, which
// then cache the flow's bucket indices of rows 0..3 (written by the claimer),
// so a packet of a known flow needs no per-row MurmurHash3; deeper sketches take
// 32-word records (one 128-byte line, as a 64-byte record's probe fetches anyway)
// whose words 12..19 cache rows 0..7.
inline uint32_t dict_record_words_cm(uint32_t K, uint32_t d) {
    const uint32_t w = 1 + (K + 3) / 4;
    return (K > 12 && w <= 12) ? (d > 4 ? 32u : 16u) : dict_record_words(K);
}

// Flow-dictionary rebuild (gns_dict.hip): keep the records whose id some
// array in `mark` names (or whose keep_nz entry is nonzero), reinsert them into
// the cleared table -- or a new one of new_slots slots -- and rewrite the ids of
// every array in `remap_arrays`.  D.rec / D.mask / slots are updated; the
// scratch's remap (old slot -> new slot, ~0 = dropped) stays valid until the
// next rebuild.  D.ctl[0] restarts at the live count.  Synchronizes stream s.
struct DictIds {
    uint32_t *ids;
    uint64_t n;
};
struct DictScratch {
    uint32_t *remap = nullptr, *stage = nullptr, *stage_slot = nullptr, *cnt = nullptr, *h_cnt = nullptr;
    uint64_t remap_n = 0, stage_n = 0;
    void free_all();
};
// grow_max != 0: the table also doubles (up to grow_max slots) while the live
// flows exceed a quarter of it.
// replace: the table is always a new allocation of new_slots slots, fewer than before
// allowed (GNS_E_FULL when the live flows pass 7/8 of them), so the old table is read only
// and a caller that passes a copy of its DictDev keeps it intact when the rebuild fails.
int dict_rebuild(DictDev &D, uint64_t &slots, const DictIds *mark, int nmark, const unsigned long long *keep_nz,
                 DictIds *remap_arrays, int nremap, uint64_t new_slots, hipStream_t s, DictScratch &sc,
                 uint64_t *live_out, uint32_t **old_rec_out, uint64_t grow_max = 0, bool replace = false);
// Keys -> flow ids, claiming the absent ones (gns_dict.hip): the write side of
// the state interface (gns_cm_import_state, gns_ss_import_state, gns_ex_merge)
// names flows by key bytes, as the exports do.  ids[i] = the slot of key i, or
// GNS_ID_NONE for a key that is not live.  The same key may occur any number of
// times.  The claim protocol is the ingest kernels' (gns_keys.cuh): a key whose
// slot was claimed in this launch is parked in its block's list and re-probed by
// the next launch, whose kernel boundary has published the key bytes; nothing is
// handed from one workgroup to another inside a launch.  The first three rounds
// are queued without a host round trip; from then on the host reads the parked
// total before each further round.
enum KeyLive {
    KEYS_ALL = 0,    // every key is live
    KEYS_CELL = 1,   // vals = u32[n]: live when a key byte or the value is nonzero (an exported sketch cell)
    KEYS_VAL64 = 2,  // vals = u64[n]: live when the value is nonzero (an exact-table row with packets)
};
// Count-Min records cache the key's row buckets in words 12.. (dict_record_words_cm); the
// claimer writes them with the key.  d == 0: no cache.
struct RowCache {
    uint32_t d = 0, w = 0, pow2 = 0, wmask = 0;
    uint32_t seeds[8] = {};
};
constexpr uint32_t kResolveChunk = 4096;      // keys per block (one parked list each)
constexpr uint64_t kResolvePiece = 1u << 20;  // most keys per call: the scratch is bounded by it
struct KeyResolveScratch {
    uint64_t *pend[2] = {nullptr, nullptr};  // [kResolvePiece] parked lists, per-block regions of kResolveChunk
    uint32_t *pcnt[2] = {nullptr, nullptr};  // [blocks] their lengths
    uint32_t *ptotal = nullptr;              // [2] parked totals of the two lists
    uint32_t *h_pin = nullptr;               // pinned host mirror of the words a round's check reads
    int reserve();
    void free_all();
};
struct KeyResolve {
    const uint8_t *keys;  // device, n * stride bytes
    uint32_t stride;
    uint64_t n;           // <= kResolvePiece
    int live;             // KeyLive
    const void *vals;     // device; see KeyLive
    uint32_t *ids;        // device [n]
    RowCache rc;
    unsigned long long *full_word;  // the engine's dictionary-full counter (raised with the abort flag)
};
// GNS_E_FULL: the claims crossed D.cap (the abort flag D.ctl[1] and *full_word are
// raised, ids are incomplete): the caller grows the table, clears *full_word and
// re-runs the call.  *claimed = D.ctl[0]; each round is timed as one launch of
// `stage` when a timer is given.  Synchronizes s.
int dict_resolve_keys(const DictDev &D, uint32_t &epoch, const KeyResolve &r, KeyResolveScratch &sc, hipStream_t s,
                      uint64_t *claimed, StageTimer *timer = nullptr, int stage = 0);

// Largest dictionary: flow ids are u32 slots below kDictMarked (0xFFFFFFFE /
// GNS_ID_NONE are reserved); 2^30 slots keep a 64-byte-record table at 64 GB.
constexpr uint64_t kDictMaxSlots = 1ull << 30;

// What an engine that recycles flow ids owns of its dictionary (Count-Min,
// SuperSpread): the table, its limits and the recovery accounting.
struct FlowDict {
    DictDev D{};
    uint64_t dict_slots = 0;
    uint64_t max_flows = 0;               // proactive reclaim once this many slots are claimed
    uint64_t claimed = 0;                 // D.ctl[0] as of the last batch
    bool full = false;                    // live flows + one batch piece exceed the largest table (sticky)
    uint32_t *dctl = nullptr;             // D.ctl: [0] claimed slots, [1] abort flag
    DictScratch dsc;                      // rebuild scratch (grow-only)
    unsigned long long *stats_bak = nullptr;  // [3] counters before the running batch (undone on abort)
    uint64_t n_reclaim = 0, n_dropped = 0, last_live = 0, n_retry = 0, n_grow = 0;
    double reclaim_ms = 0.0;

    // claims beyond 3/4 load abort the batch; proactive reclaim at load 1/2
    void limits();
    // Rebuild keeping the flows that `ids` name (and remapping them).  The table
    // doubles while the live flows exceed a quarter of it, and to at least min_slots.
    int reclaim(DictIds *ids, int n, uint64_t min_slots, hipStream_t s);
    void stats(uint64_t out[8]) const;  // gns_*_dict_stats
    void free_all();
};

// Engine counters [0..2] saved before a batch runs and restored when it aborts
// (clear_full: with the dictionary-full word [3] the abort raised).
int stats_save(unsigned long long *bak, const unsigned long long *stats, hipStream_t s);
int stats_undo(unsigned long long *stats, const unsigned long long *bak, bool clear_full, hipStream_t s);

// One device batch (device-resident inputs) with dictionary recovery: a batch
// whose new flows overflow the dictionary is aborted before it changes the
// engine's state, its counters are undone and its claims dropped with the dead
// flows (reclaim); it is re-run as is once, then in halves.  A piece of <= chunk
// records that does not fit a freshly rebuilt dictionary doubles the table
// instead, so the engine keeps counting whatever the stream brings: live ids are
// bounded by the engine's cells, the table by kDictMaxSlots.
struct DictRecovery {
    FlowDict &fd;
    unsigned long long *stats;
    hipStream_t stream;
    uint64_t chunk;      // halves are whole chunks
    const char *piece;   // what the last error message calls a piece that cannot fit
    std::function<int(const InputDesc &, uint64_t)> run;  // one batch; may itself split through batch()
    std::function<int(uint64_t)> reclaim;                 // the engine's reclaim (min_slots)
    // fresh: the dictionary was rebuilt right before this batch
    int batch(const InputDesc &d, uint64_t m, bool fresh) const;
};

// --- the read side ---------------------------------------------------------
// Device bytes -> pageable host memory through two pinned chunks, one in flight while
// the other is copied out: a copy to pageable memory blocks in the runtime, which may
// not happen under a reader while the handle ingests.  (The arithmetic: gns_pinchunk.hpp.)
constexpr size_t kPinChunk = 4u << 20;
struct PinnedOut {
    uint8_t *pin = nullptr;
    size_t pin_n = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};  // a chunk's copy has landed
    // at least `bytes` of pinned memory (grow-only, to twice the request, never below two
    // chunks) and the events
    int reserve(size_t bytes);
    // complete on return.  sw != 0: rows of sw source bytes of which the first dw go out
    int copy_out(void *dst, const void *src, size_t bytes, hipStream_t s, size_t sw = 0, size_t dw = 0);
    // host bytes -> device through the two halves, one being filled while the other's copy runs.
    // Complete on return (synchronizes s).
    int copy_in(void *dst, const void *src, size_t bytes, hipStream_t s);
    void free_all();
};

// Grow-only device staging of a host point query's keys and answers: no allocation or
// free -- hipFree synchronizes the device -- once warm.  pin: host keys and answers
// pass through that pinned memory (a view's: see PinnedOut).
struct QueryStage {
    uint8_t *qkeys = nullptr;
    uint64_t *qout = nullptr;
    uint64_t qkeys_n = 0, qout_n = 0;
    PinnedOut *pin = nullptr;
    void free_all();
};
// The point query of every engine and view: n keys of key_bytes at `stride` -> out[n],
// host memory or (dev) device memory, where the call returns once the answers are
// written.  launch(dk, dout) enqueues the engine's kernel on s over the device keys
// and answers; the checks, the staging, the sync and the error mapping are here.
using LaunchFn = std::function<int(const uint8_t *dk, uint64_t *dout)>;
int query_keys(int device, hipStream_t s, QueryStage &st, const char *what, const uint8_t *keys, uint32_t stride,
               uint32_t key_bytes, uint64_t n, uint64_t *out, bool dev, const LaunchFn &launch);

// What a snapshot view owns besides its copy of the state: a stream of the device's
// highest priority (a reader's small launches are dispatched ahead of the ingest
// pipeline's queued workgroups), the event that orders it behind a refresh, and the
// mutex between refresh and readers (a refresh waits for the reader call in progress).
struct ViewCore {
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr;
    std::mutex mu;
    int init();
    // what is queued on the handle's stream so far is the view's state: readers wait for it
    int publish(hipStream_t handle_stream);
    void quiesce();  // destroy: waits for the reader call in progress (its stream is synchronized)
    void destroy();
};

// gns_frame.cpp: one captured frame -> one 64-byte record for the device
// parser.  Returns 0 = copied verbatim (device fast-path shape), 1 = decoded
// into a pre-parsed 0x88B5 record, 2 = no IP layer (a record the device drops).
int frame_record(const uint8_t *frame, uint32_t caplen, uint32_t wirelen, uint8_t *rec);
// frame_record's record (and its return code) -> compact 16-byte record; returns
// the class (kRecSide: the caller stores the side index in word 0)
int compact_record(int code, const uint8_t *rec, uint8_t *out16);
// the 16-byte form: the wire length in word 3 bits 16..31 (-1: above 65535); a tuple
// record is IPv4 both ways, any other tuple escapes to the side array
int compact_record16(int code, const uint8_t *rec, uint32_t orig, uint8_t *out16);

inline uint32_t ceil_log2(uint64_t x) {
    uint32_t b = 0;
    while ((1ull << b) < x) b++;
    return b;
}

}  // namespace gns
