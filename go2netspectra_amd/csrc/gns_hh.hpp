// gns_hh.hpp -- the device heavy-hitter list (gns_hh.hip) shared by Count-Min,
// SuperSpread, the exact spread engine and the multi-GPU row merge
// (gns_hh_order_rows): the list's scratch, and its host entry points.
//
// One (value, fingerprint id) cell array whose ids are slots of a flow dictionary
// -> the list of flows whose max over their cells reaches `thr`, in canonical order
// (value desc, flow bytes asc): candidate compaction, per-flow max + one emit per
// flow, the hand-written LSD radix order, one D2H.  count_min.go:178-247 and
// super_spread.go:254-294 are both this computation (a flow's estimate is the max
// over the cells that hold it, so it reaches thr iff one of those cells does).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gns_keys.cuh"

namespace gns {

// Grow-only device / pinned buffers of the list: no allocation or free --
// hipFree synchronizes the device -- once warm, so a snapshot view can list
// while the handle ingests.
struct HhScratch {
    uint64_t *cand = nullptr;
    uint32_t *ncand = nullptr;
    uint64_t cap = 0;               // candidates cand holds
    uint8_t *bytes = nullptr;       // id -> key bytes (the list's entries, hh_ids_to_host_bytes)
    uint64_t bytes_n = 0;
    // per-flow-id max / mark words (dense over the dictionary's slots, epoch-tagged so
    // they are never cleared), unique (id, value), order indices, radix-pass histograms
    // (block-major) and their scan
    unsigned long long *best = nullptr;
    uint32_t *mark = nullptr;
    uint64_t best_n = 0, mark_n = 0;
    uint32_t hh_epoch = 0;
    uint32_t *u32a = nullptr, *u32b = nullptr, *u32c = nullptr, *u32d = nullptr;
    uint64_t u32a_n = 0, u32b_n = 0, u32c_n = 0, u32d_n = 0;
    uint32_t *rsh = nullptr;    // [blocks][256] histograms, then [ngrp][256] group sums, [256] totals, total, tie flag
    uint64_t rsh_n = 0;
    uint8_t *obytes = nullptr;  // ordered flow bytes
    uint64_t obytes_n = 0;
    uint8_t *hpin = nullptr;    // pinned host staging of the rows (D2H into pageable
    uint64_t hpin_n = 0;        // caller memory went through the runtime's slow path)
    uint32_t *hsm = nullptr;    // pinned host words for the list's small read-backs (lengths, flags):
                                // a 4-byte D2H into a pageable stack word took 28-35 ms now and then
    void free_all();
};

// The list's buffers sized up front (a handle's or a view's create), so a
// window's first call allocates nothing: candidates for min(cells, 4M) buckets,
// the per-flow words for the dictionary's slots, unique entries and their order
// for 1M flows.  Larger lists still grow them.
int hh_reserve(HhScratch &sc, uint64_t cells, uint64_t slots, uint32_t K, hipStream_t st);
// The list of one cell array of `cells` cells.  flows: n*K bytes, vals: n values;
// *n_io = capacity in, full list length out.  rows_dev non-null: the ordered list
// as packed device rows [flow | u32 value] (capacity *n_io rows), no host copy.
// Runs on stream st and returns after the list is written.
int hh_heavy_list(HhScratch &sc, hipStream_t st, const DictDev &D, uint64_t dict_slots, uint32_t K, uint64_t cells,
                  const uint32_t *val, const uint32_t *fp, uint32_t thr, uint8_t *flows, uint32_t *vals,
                  uint64_t *n_io, uint8_t *rows_dev = nullptr);
// flow ids -> key bytes in host memory (GNS_ID_NONE -> zero bytes, the reference's reset FP)
int hh_ids_to_host_bytes(HhScratch &sc, hipStream_t st, const DictDev &D, const uint32_t *d_ids, uint64_t n,
                         uint8_t *host);
// the same into device memory (n * D.K bytes), enqueued on st: a view's chunked export
int hh_ids_to_dev_bytes(hipStream_t st, const DictDev &D, const uint32_t *d_ids, uint64_t n, uint8_t *d_out);
// The canonical order (value desc, flow bytes asc) of n packed device rows [flow (K) | u32
// value] -> out_rows (device, not `rows`), with the caller's scratch on stream st: enqueued,
// no copy to the host, the stream is not synchronized at the end (gns_hh_order_rows is this
// on the null stream with a per-thread scratch).
int hh_order_rows_dev(HhScratch &sc, hipStream_t st, const uint8_t *rows, uint32_t K, uint32_t n, uint8_t *out_rows);
}  // namespace gns
