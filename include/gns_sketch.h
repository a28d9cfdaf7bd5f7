/*
 * gns_sketch.h -- C ABI of the MI355X sketch engine (libgns_sketch.so).
 *
 * Drop-in boundary for Go2NetSpectra's sketch hot path.  Each entry point names
 * the reference interface it replaces (paths relative to the reference repo):
 *
 *   statistic.Sketch.Insert(flow, elem, size)  internal/engine/impl/sketch/statistic/sketch.go:6
 *       -> gns_cm_insert_keys / gns_ss_insert_keys           (batched, stream-ordered)
 *   sketch.Task.ProcessPacket(*PacketInfo)     internal/engine/impl/sketch/task.go:156-169
 *       -> gns_cm_insert_tuples / gns_ss_insert_tuples       (EncodeFlow fused on device)
 *   pcap.Reader.ReadPackets + ParsePacketInto  pkg/pcap/reader.go:35-49, internal/protocol/parser.go:23-67
 *       -> gns_cm_insert_headers / gns_ss_insert_headers     (64-byte records, parse fused)
 *   statistic.Sketch.Query(flow)               sketch.go:7; count_min.go:160-174; super_spread.go:238-249
 *       -> gns_cm_query / gns_ss_query
 *   statistic.Sketch.HeavyHitters()            sketch.go:8; count_min.go:178-247; super_spread.go:254-294
 *       -> gns_cm_heavy_hitters / gns_ss_heavy_hitters
 *   statistic.Sketch.Reset()                   sketch.go:9; count_min.go:249-265; super_spread.go:297-311
 *       -> gns_cm_reset / gns_ss_reset
 *   statistic.NewCountMin / NewSuperSpread     count_min.go:47-90; super_spread.go:127-179
 *       -> gns_cm_create / gns_ss_create (seeds injected, see below)
 *
 * Rules:
 *   - Every call returns GNS_OK (0) or a negative gns_status; gns_last_error()
 *     returns the thread-local message of the last failure.
 *   - Calls on one handle must be serialized by the caller (one goroutine per
 *     handle).  Inserts are applied in call order, packets in array order:
 *     the device state equals the reference sketch fed the same stream by ONE
 *     worker (num_workers: 1) with the same seeds.
 *   - Pointers flagged GNS_MEM_HOST are read before the call returns (the
 *     caller keeps ownership).  GNS_MEM_DEVICE pointers must be device memory
 *     of the handle's device and stay valid until gns_*_flush() returns.
 *   - Flow keys are the reference EncodeFlow bytes (task.go:279-300): IP slots
 *     of 16 bytes with IPv4 left-aligned and zero padded, ports big-endian,
 *     protocol one byte; key_bytes <= 37 (task.go:74).
 *   - Flow dictionary (fingerprints are dense flow ids): the
 *     reference's buckets hold key bytes (count_min.go:66-81), so Insert has no
 *     failure mode whatever the traffic (count_min.go:94-157).  Here a bucket
 *     names a dictionary slot; between device batches the sketches reclaim the
 *     flows no bucket names any more and the table DOUBLES while the live flows
 *     exceed a quarter of it (live ids are at most 2*depth*width for Count-Min,
 *     depth*width for SuperSpread).  A batch whose new flows overflow the table
 *     is not applied: the dictionary is rebuilt and the batch re-run (in
 *     halves; a piece of 16K packets that still does not fit grows the table).
 *     max_flows is only the INITIAL capacity.  GNS_E_FULL is left only for a
 *     table of 2^30 slots (64 GB of 64-byte records) that cannot take one 16K
 *     piece next to its live flows -- beyond any sketch with depth*width <=
 *     2^27 -- and then holds until gns_*_reset() (the period reset,
 *     manager.go:179-193).  The exact aggregator's table grows the same way.
 *   - Sizes >= 2^16-1 take an overflow side table that grows with the batch
 *     (no per-batch limit).
 *   - Deviations from NewCountMin (count_min.go:47-60), which accepts any
 *     geometry: depth <= 8 (GNS_E_ARG) and width < 2^25 (GNS_E_RANGE; at depth
 *     8 also width <= 2^25 / bins limit, see gns_cm_create's message).  Batches
 *     are capped at 2^31 / depth packets (longer inserts are split).
  */
#ifndef GNS_SKETCH_H
#define GNS_SKETCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gns_status {
    GNS_OK = 0,
    GNS_E_ARG = -1,    /* bad argument (log.Fatalf / panic sites in the reference) */
    GNS_E_HIP = -2,    /* HIP runtime error */
    GNS_E_OOM = -3,    /* device allocation failed */
    GNS_E_FULL = -4,   /* flow dictionary at its 2^30-slot limit (see the rules above) */
    GNS_E_RANGE = -5,  /* geometry beyond a documented limit (see message) */
    GNS_E_NODEV = -6   /* no usable HIP device */
} gns_status;

typedef enum gns_mem { GNS_MEM_HOST = 0, GNS_MEM_DEVICE = 1 } gns_mem;

/* gns_*_set_timing(h, GNS_TIMING_MASK | stage bits): time only those stages */
#define GNS_TIMING_MASK 0x100

/* task.go:279-300 field names -> ids; fieldByteSize task.go:327-338 */
typedef enum gns_field {
    GNS_F_NONE = 0, GNS_F_SRCIP = 1, GNS_F_DSTIP = 2, GNS_F_SRCPORT = 3, GNS_F_DSTPORT = 4,
    GNS_F_PROTO = 5
} gns_field;

typedef struct gns_layout {
    uint32_t n_fields;
    uint8_t fields[8]; /* gns_field, in configured order (SketchTaskDef.FlowFields) */
} gns_layout;

/* Pre-parsed packets: model.PacketInfo (internal/model/packet.go:9-22) as SoA.
 * src16/dst16 hold the 16-byte slots exactly as EncodeFlow lays them out. */
typedef struct gns_tuples {
    const uint8_t *src16;   /* n*16 */
    const uint8_t *dst16;   /* n*16 */
    const uint16_t *sport;  /* n */
    const uint16_t *dport;  /* n */
    const uint8_t *proto;   /* n */
    const uint32_t *length; /* n, uint32(PacketInfo.Length) (task.go:168) */
} gns_tuples;

/* ------------------------------------------------------------------ */
/* Count-Min (count_min.go)                                           */
/* ------------------------------------------------------------------ */
typedef struct gns_cm gns_cm;

typedef struct gns_cm_params {
    uint32_t width, depth;                    /* 0 -> 2^20 / 3 (count_min.go:48-53) */
    uint32_t size_threshold, count_threshold; /* 0 -> 512 KiB / 512 (count_min.go:54-59) */
    gns_layout flow;                          /* flow key layout (for tuples/headers input) */
    uint32_t key_bytes;                       /* FS; must equal the layout's byte size when
                                                 n_fields > 0; used alone for keys input */
    const uint32_t *seeds;                    /* depth row seeds (count_min.go:61-64 draws
                                                 them with rand.Uint32; here injected).
                                                 NULL -> splitmix64(0x9747B28C) stream */
    uint64_t max_flows;                       /* INITIAL flow dictionary capacity (it grows with
                                                 the live flows; dead flows are reclaimed); 0 -> 4M */
    uint64_t batch_packets;                   /* device batch size; 0 -> 16M packets */
    int device;                               /* HIP device ordinal */
    uint32_t bucket_lo, bucket_hi;            /* bucket-range slice (SURVEY §8e exact global
                                                 mode): only updates whose row bucket lies in
                                                 [bucket_lo, bucket_hi) are applied, so G handles
                                                 fed the same stream with disjoint ranges hold,
                                                 between them, exactly the state of one handle.
                                                 0, 0 -> the whole row */
} gns_cm_params;

int gns_cm_create(const gns_cm_params *p, gns_cm **out);
int gns_cm_destroy(gns_cm *cm);
/* statistic.Sketch.Insert batch: keys[n*stride] (first key_bytes used), sizes[n] */
int gns_cm_insert_keys(gns_cm *cm, const uint8_t *keys, uint32_t stride, const uint32_t *sizes,
                       uint64_t n, gns_mem where);
/* Task.ProcessPacket batch over pre-parsed PacketInfo */
int gns_cm_insert_tuples(gns_cm *cm, const gns_tuples *t, uint64_t n, gns_mem where);
/* fused parse: hdr[n*64] = first 64 bytes of each frame (zero padded),
 * wirelen[n] = capture orig_len (= PacketInfo.Length, parser.go:30-33).
 * Records outside the device parser's subset (gns_device.cuh parse_record:
 * Ethernet II, <= 2 VLAN tags, IPv4 without options, IPv6 without extension
 * headers, TCP/UDP, no tunnels) are skipped and counted (gns_cm_stats [2]);
 * the host packer (gns_pack_pcap) never emits them: it decodes such frames
 * itself (gns_frame_record). */
int gns_cm_insert_headers(gns_cm *cm, const uint8_t *hdr, const uint32_t *wirelen, uint64_t n,
                          gns_mem where);
/* Compact records (the PCIe-bound host-inclusive path): rec16[n*16]
 * = the canonical tuple the device parser derives from a 64-byte record, in 16
 * bytes + wirelen[n] (20 B/packet instead of 68):
 *   word 0 IPv4 source, word 1 IPv4 destination (the left-aligned slots' first
 *   4 bytes), word 2 ports (big-endian bytes), word 3 = protocol | class << 8 |
 *   destination IP version << 16 | source IP version << 24;
 *   class 0 = that tuple, 1 = no IP layer (not counted, parser.go:48-49),
 *   2 = escape: word 0 indexes side64[n_side*64], a 64-byte record parsed as
 *   gns_cm_insert_headers parses it (IPv6 tuples, unsupported shapes).
 * The insert equals gns_cm_insert_headers of the records the compact form was
 * made from.  Producers: gns_pack_pcap_compact (host), gns_compact_headers (device).
 * wirelen == NULL: the 16-byte form (16 B/packet over the bus): word 3 bits 16..31
 * hold the wire length instead of the IP versions, a class-0 record is an IPv4
 * tuple both ways (any other tuple escapes to side64), so no wire lengths above
 * 65535; producers gns_pack_pcap_compact16, gns_compact_headers16. */
int gns_cm_insert_compact(gns_cm *cm, const uint8_t *rec16, const uint32_t *wirelen, uint64_t n,
                          const uint8_t *side64, uint64_t n_side, gns_mem where);
int gns_cm_flush(gns_cm *cm);
/* out[i] = count<<32 | size, count_min.go:160-174 */
int gns_cm_query(gns_cm *cm, const uint8_t *keys, uint32_t stride, uint64_t n, uint64_t *out);
/* gns_cm_query with keys and out in DEVICE memory of the handle's GPU (out 8-byte
 * aligned): the owner-routed query path keeps keys and answers on the GPU between
 * its all-to-alls.  The keys must be complete when called; returns once out is written. */
int gns_cm_query_device(gns_cm *cm, const uint8_t *keys, uint32_t stride, uint64_t n, uint64_t *out);
/* HeavyHitters, count_min.go:178-247.  Lists are sorted value-descending with
 * ties broken by flow bytes ascending (the reference leaves ties unordered).
 * On input *n_count / *n_size hold the capacities (entries); on output the
 * full list lengths (call again with larger buffers if they exceed the
 * capacities).  flows_* are n*key_bytes. */
int gns_cm_heavy_hitters(gns_cm *cm, uint8_t *count_flows, uint32_t *counts, uint64_t *n_count,
                         uint8_t *size_flows, uint32_t *sizes, uint64_t *n_size);
/* HeavyHitters into DEVICE memory, for the multi-GPU window exchange (the lists
 * stay on the device through the all-gather and the merge): packed rows
 * [flow (key_bytes) | value (u32, little-endian)], in the order above;
 * *n_count / *n_size in/out as for gns_cm_heavy_hitters (capacities in rows; a
 * list longer than its buffer is reported and not written). */
int gns_cm_heavy_rows(gns_cm *cm, uint8_t *count_rows, uint64_t *n_count, uint8_t *size_rows, uint64_t *n_size);
/* The canonical order (value desc, flow bytes asc) of n DEVICE rows of the form
 * above -- the union of flow-disjoint per-shard lists after an all-gather
 *  -- written to out_rows (device).  Runs on the device's null
 * stream, ordered after the caller's earlier work on it; returns when done. */
int gns_hh_order_rows(const uint8_t *rows, uint32_t key_bytes, uint64_t n, uint8_t *out_rows, int device);
int gns_cm_reset(gns_cm *cm);
/* Full state for parity: C/S [depth*width], FPc/FPs [depth*width*key_bytes]
 * (any pointer may be NULL). */
int gns_cm_export_state(gns_cm *cm, uint32_t *C, uint32_t *S, uint8_t *FPc, uint8_t *FPs);
/* Restore: replace the handle's whole state by the arrays gns_cm_export_state
 * writes (host pointers, all four required; layout as there).  counters: NULL =
 * leave gns_cm_counters' [0..2] as they are, else their new values.
 *   - The call equals gns_cm_reset followed by whatever inserts produced the
 *     arrays: gns_cm_export_state then returns the same bytes, queries and both
 *     heavy-hitter lists answer as the exporting handle's did, and every later
 *     insert leaves the state bit-equal to the sequential reference continued from
 *     that state.  The arrays must come from a sketch of the same geometry, key
 *     width and row seeds; the call cannot detect any other.
 *   - A cell is live when its fingerprint bytes are non-zero or its value is
 *     non-zero.  C == 0 with a live FPc (count_min.go:145-151) and S == 0 with a
 *     live FPs (:121-125) are legal states and survive the round trip; a zero
 *     fingerprint with a zero value is the empty cell.
 *   - Derived structures: the flow dictionary is rebuilt from the distinct
 *     fingerprints on the device (bucket cache included; the table grows as for
 *     ingest), the hot-bucket designation is cleared (the next batch re-picks it;
 *     results do not depend on it), the error words [3], [4] and [9] are cleared.
 *   - Snapshot views are quiesced and the period is bumped: a view taken before
 *     the import answers GNS_E_ARG until refreshed, as after gns_cm_reset.
 *   - GNS_E_ARG (a null pointer) leaves the handle untouched; any later error
 *     leaves it as after gns_cm_reset.
 * With gns_cm_set_timing on, stage 0 times the host-to-device staging and stage 1
 * the resolve rounds (one launch each).  The exact spread aggregator (gns_exs_*)
 * has no import: its pair set is not exportable, only per-flow counts are. */
int gns_cm_import_state(gns_cm *cm, const uint32_t *C, const uint32_t *S, const uint8_t *FPc, const uint8_t *FPs,
                        const uint64_t *counters /* [3] or NULL */);
/* stats[0]=packets inserted, [1]=records dropped (not IP), [2]=records outside
 * the fast-parse subset, [3]=distinct flows in the dictionary */
int gns_cm_stats(gns_cm *cm, uint64_t stats[4]);
/* Per-stage device time (ms, HIP events on the handle's stream), accumulated
 * since the last call with reset != 0.  Stages: 0 extract, 1 resolve, 2 scan,
 * 3 scatter, 4 apply, 5 total insert, 6 hot-bucket aggregate/decide/fallback,
 * 7 hot-bucket designation.  Enabled by gns_cm_set_timing(cm, 1) (every stage) or
 * gns_cm_set_timing(cm, GNS_TIMING_MASK | bits) (only the stages whose bits are set: each
 * timed stage puts two events into the batch's stream). */
/* raw engine counters: [0] inserted, [1] dropped, [2] unsupported, [3] dictionary
 * full, [4] size-overflow full, [5] tile updates replayed sequentially,
 * [6] tile chunks, [7] tile chunks with a replay */
int gns_cm_counters(gns_cm *cm, uint64_t out[8]);
/* flow dictionary: [0] reclaims, [1] dead flows dropped, [2] live flows after the
 * last reclaim, [3] claimed slots now, [4] reclaim time (us, host clock incl. the
 * rebuild's device work), [5] batches re-run after a dictionary overflow,
 * [6] dictionary slots now, [7] table growths */
int gns_cm_dict_stats(gns_cm *cm, uint64_t out[8]);
/* reclaim now (e.g. at a window boundary; inserts also reclaim on their own) */
int gns_cm_reclaim(gns_cm *cm);
int gns_cm_set_timing(gns_cm *cm, int on);
int gns_cm_stage_times(gns_cm *cm, double ms[8], uint64_t launches[8], int reset);
void *gns_cm_stream(gns_cm *cm); /* hipStream_t the handle launches on */

/* Snapshot view: heavy hitters and queries CONCURRENT with ingest (BASELINE
 * configs[4]; the reference's snapshotter and alerter call Task.Snapshot ->
 * HeavyHitters while the workers insert, manager.go:139-159, task.go:177).
 *   - gns_cm_view_refresh is an ingest-side call (serialized with the handle's
 *     other calls): it copies the bucket state, in insert order, at the current
 *     end of the insert stream (a window boundary), asynchronously on the
 *     handle's stream.
 *   - gns_cm_view_heavy_hitters / gns_cm_view_query may run on any other
 *     thread while the handle keeps inserting; they run on the view's own
 *     stream and see exactly the state at the last refresh (same results as
 *     gns_cm_heavy_hitters / gns_cm_query called at that point).
 *   - A refresh waits for a view call in progress; after gns_cm_reset the view
 *     answers GNS_E_ARG until it is refreshed.  Destroy views before their handle.
 * Memory: 16 bytes per bucket (depth*width) for the snapshot. */
typedef struct gns_cm_view gns_cm_view;
int gns_cm_view_create(gns_cm *cm, gns_cm_view **out);
int gns_cm_view_destroy(gns_cm_view *v);
int gns_cm_view_refresh(gns_cm_view *v);
int gns_cm_view_heavy_hitters(gns_cm_view *v, uint8_t *count_flows, uint32_t *counts, uint64_t *n_count,
                              uint8_t *size_flows, uint32_t *sizes, uint64_t *n_size);
int gns_cm_view_query(gns_cm_view *v, const uint8_t *keys, uint32_t stride, uint64_t n, uint64_t *out);

/* Detached snapshot: gns_cm_view_refresh_at(v, GNS_CM_VIEW_DETACH) resolves what
 * the view needs out of the flow dictionary at the refresh, so that afterwards
 * nothing in the view points into the handle (the reference's resetter runs
 * independently of its snapshotter, manager.go:161-193 against :116-159: list a
 * window's heavy hitters from another thread while the handle has already been
 * reset and counts the next window).  flags == 0 is gns_cm_view_refresh.
 *   - Refresh.  An ingest-side call like gns_cm_view_refresh, everything enqueued
 *     on the handle's stream, no host synchronization: every flow id a bucket
 *     names is marked (one word per dictionary slot), the marked slots are counted
 *     and scanned into dense indices in slot order, their records {tag, key words}
 *     are gathered into the view's compact key table (row `dense`), and the view's
 *     fingerprint arrays hold dense indices instead of slots (GNS_ID_NONE kept).
 *     The counters and the handle's counters [0..2] are copied with them.  The
 *     view's buffers are grow-only and sized from host-known bounds: the
 *     dictionary's slots for the mark / remap words, the claimed slots (at most
 *     2*depth*width) for the table.  A refresh that outgrows them allocates (and
 *     frees, which synchronizes the device); any other refresh allocates nothing.
 *     It takes the view's mutex, so it waits for a reader call in progress.
 *   - Readers.  gns_cm_view_heavy_hitters, gns_cm_view_query and the three calls
 *     below run on the view's own stream with its own grow-only scratch and pinned
 *     staging.  On a detached snapshot they read no handle state: a fingerprint
 *     matches a key iff the cell's dense id is not GNS_ID_NONE and the table row's
 *     key words equal the key's (an empty cell never matches, the all-zero key
 *     included).  Every answer is what the handle's call would have answered at
 *     the refresh: gns_cm_view_query[_device] = gns_cm_query[_device];
 *     gns_cm_view_heavy_hitters = gns_cm_heavy_hitters (canonical order, capacity
 *     rule); gns_cm_view_heavy_rows = gns_cm_heavy_rows (packed DEVICE rows; a
 *     list longer than *n is reported and not written; a NULL array with *n == 0
 *     asks for the length); gns_cm_view_export_state = gns_cm_export_state plus
 *     gns_cm_counters' [0..2].  On a plain snapshot the three calls go through the
 *     live dictionary and obey the stale rule above; `counters` of a plain
 *     snapshot is GNS_E_ARG before any device call.  Null outputs are skipped.
 *   - Lifetime.  A detached snapshot is NOT staled by gns_cm_reset,
 *     gns_cm_reclaim, dictionary growth or gns_cm_import_state: it answers the
 *     refresh-point state until the next refresh, and those calls do not wait for
 *     a reader call in progress on it.  A reclaim neither remaps it nor keeps the
 *     flows alive that only it names.  A plain refresh of the same view brings
 *     back the plain behaviour exactly.  Several views of one handle are
 *     independent.
 *   - Errors.  A null view, a null out (n > 0), a null n_count / n_size and
 *     stride < key_bytes are GNS_E_ARG before any device call; so are unknown
 *     flags.  A bucket whose id named no dictionary slot at the refresh (corrupt
 *     state) is not dereferenced; the next reader call answers GNS_E_HIP.
 * Memory of a detached snapshot: the plain 16 bytes per bucket, 4 bytes per
 * dictionary slot, one 64-byte record row (16 bytes for keys up to 12 bytes) per
 * live flow, and the scan's words (about 4 bytes per 256 slots). */
#define GNS_CM_VIEW_DETACH 1u
int gns_cm_view_refresh_at(gns_cm_view *v, uint32_t flags);
int gns_cm_view_query_device(gns_cm_view *v, const uint8_t *keys, uint32_t stride, uint64_t n, uint64_t *out);
int gns_cm_view_heavy_rows(gns_cm_view *v, uint8_t *count_rows, uint64_t *n_count, uint8_t *size_rows,
                           uint64_t *n_size);
int gns_cm_view_export_state(gns_cm_view *v, uint32_t *C, uint32_t *S, uint8_t *FPc, uint8_t *FPs,
                             uint64_t *counters /* [3] */);

/* ------------------------------------------------------------------ */
/* SuperSpread (super_spread.go)                                      */
/* ------------------------------------------------------------------ */
typedef struct gns_ss gns_ss;

typedef struct gns_ss_params {
    uint32_t width, depth, threshold;  /* 0 -> 2^20 / 3 / 4096 (super_spread.go:12-20) */
    uint32_t m, size;                  /* 0 -> 128 / 5; size <= 8 */
    double base, b;                    /* 0 -> 0.5 / 1.08 */
    gns_layout flow, elem;             /* FlowFields / ElementFields */
    uint32_t flow_bytes, elem_bytes;
    const uint32_t *seeds;             /* depth row seeds (super_spread.go:175); NULL -> default */
    uint64_t hll_master;               /* derives each GeneralHLL's seeds[0..1] */
    uint64_t rng_seed;                 /* keys the declared generator replacing rand.Float64 */
    uint64_t batch_packets;
    uint64_t max_flows;                /* initial flow dictionary capacity (grows); 0 -> 4M */
    int device;
} gns_ss_params;

/* The SuperSpread flow dictionary holds the flows that own a cell (only they
 * can be named by a key, a query or a heavy hitter); it is reclaimed and grows
 * like Count-Min's (see the rules above), so inserts do not fail on it.
 * Deviations (GNS_E_ARG at create): depth <= 8, m <= 256, size <= 8, merged
 * key <= 74 bytes, depth * width <= 2^25 cells.  A device batch in which one
 * cell gets more than 8192 encodes (possible with m = 256 only) is undone before
 * any state write and re-run in halves (a cell takes at most one encode per
 * record), so inserts do not fail on it. */
int gns_ss_create(const gns_ss_params *p, gns_ss **out);
int gns_ss_destroy(gns_ss *ss);
int gns_ss_insert_keys(gns_ss *ss, const uint8_t *flows, uint32_t fstride, const uint8_t *elems,
                       uint32_t estride, uint64_t n, gns_mem where);
int gns_ss_insert_tuples(gns_ss *ss, const gns_tuples *t, uint64_t n, gns_mem where);
int gns_ss_insert_headers(gns_ss *ss, const uint8_t *hdr, const uint32_t *wirelen, uint64_t n,
                          gns_mem where);
/* Compact records, by the contract of gns_cm_insert_compact: the insert equals
 * gns_ss_insert_headers of the 64-byte records the compact form was made from
 * (state, counters [0..2], the declared generator's record index).  wirelen ==
 * NULL: the 16-byte form.  Class 1 records are dropped and counted in [1]; an
 * escape whose index is at or past n_side is counted unsupported in [2] and its
 * side record never read; escapes index the side array of the whole call; every
 * array of a call lives in `where`.  GNS_E_ARG before any device call for a null
 * handle, a null rec16 with n > 0, and n_side > 0 with a null side64.  Device
 * arrays must stay valid until the call returns (the flow ids of the batch's
 * encodes are derived from them after the sort). */
int gns_ss_insert_compact(gns_ss *ss, const uint8_t *rec16, const uint32_t *wirelen, uint64_t n,
                          const uint8_t *side64, uint64_t n_side, gns_mem where);
int gns_ss_flush(gns_ss *ss);
int gns_ss_query(gns_ss *ss, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
/* device keys / answers, as gns_cm_query_device */
int gns_ss_query_device(gns_ss *ss, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
int gns_ss_heavy_hitters(gns_ss *ss, uint8_t *flows, uint32_t *spreads, uint64_t *n);
int gns_ss_reset(gns_ss *ss);
/* values[d*w], keys[d*w*flow_bytes], regs[d*w*m] (u8), pbits[d*w] */
int gns_ss_export_state(gns_ss *ss, uint32_t *values, uint8_t *keys, uint8_t *regs, double *pbits);
/* Restore from the arrays gns_ss_export_state writes (host pointers, all
 * required), as gns_cm_import_state.  records = the declared generator's
 * position, gns_ss_counters' [6] (records since create, dropped ones included):
 * it is part of the state -- without it a restored sketch draws other uniforms.
 * counters: NULL or the new [0..2].  pbits is taken as bit patterns.  A cell's key
 * is live when its bytes or its value are non-zero.  A key in a cell it does not
 * hash to -- no stream produces one -- is never read by a query but counts in
 * gns_ss_heavy_hitters (a flow's max over the cells that hold it).  A register
 * above 2^size - 1 is GNS_E_ARG: it would index past the power tables; the check
 * runs on the device before any state is written, and the handle stays untouched
 * (as for a null pointer).  Any later error leaves the handle as after gns_ss_reset. */
int gns_ss_import_state(gns_ss *ss, const uint32_t *values, const uint8_t *keys, const uint8_t *regs,
                        const double *pbits, uint64_t records, const uint64_t *counters /* [3] or NULL */);
int gns_ss_stats(gns_ss *ss, uint64_t stats[4]);
/* out[8]: inserted, dropped, unsupported, dictionary full, HLL candidates
 * (lz above the batch-entry register), HLL encodes, records, device batches */
int gns_ss_counters(gns_ss *ss, uint64_t out[8]);
int gns_ss_dict_stats(gns_ss *ss, uint64_t out[8]);  /* as gns_cm_dict_stats */
int gns_ss_reclaim(gns_ss *ss);
int gns_ss_set_timing(gns_ss *ss, int on);
int gns_ss_stage_times(gns_ss *ss, double ms[8], uint64_t launches[8], int reset);

/* Snapshot view: the list, queries and the whole state (a checkpoint) read
 * CONCURRENTLY with ingest, at a defined point of the stream (the reference's
 * snapshotter and alerter call Task.Snapshot while the workers insert,
 * manager.go:139-159, sketch/task.go:177,187-243).  A view holds, per cell, the
 * value and the owner's key bytes resolved at the refresh; nothing in it points
 * into the handle.
 *   - Refresh.  gns_ss_view_refresh is an ingest-side call, serialized by the
 *     caller with the handle's other calls.  Everything is enqueued on the
 *     handle's stream: the snapshot is exactly the state after every insert
 *     issued so far and before any later one.  An event behind it is what the
 *     view's stream waits for.  It makes no host synchronization; after the first
 *     refresh of each kind (with / without GNS_SS_VIEW_STATE) it allocates nothing.
 *     It takes the view's mutex, so it waits for a reader call in progress.  With
 *     gns_ss_set_timing on, stage 6 of gns_ss_stage_times is its device time.
 *   - Readers (every other call but create / destroy) may run on any thread while
 *     the handle inserts.  They run on the view's own stream, created at the
 *     device's highest priority, with the view's own grow-only scratch and pinned
 *     staging: once warm, no hipFree and no copy to or from pageable memory.
 *   - Results.  Every answer is what the handle's call would have answered at the
 *     refresh: gns_ss_view_query[_device] = gns_ss_query[_device] (max(1, .) for
 *     an absent flow included); gns_ss_view_heavy_hitters = gns_ss_heavy_hitters,
 *     the same list in the same canonical order (estimate desc, flow bytes asc)
 *     with the same capacity rule (*n: capacity in, full length out, no row at or
 *     past the capacity is written); gns_ss_view_heavy_rows = that list as packed
 *     DEVICE rows [flow | u32], as gns_cm_heavy_rows (a list longer than *n is
 *     reported and not written; rows_dev NULL asks for the length);
 *     gns_ss_view_export_state = gns_ss_export_state plus gns_ss_counters' [6]
 *     (records) and [0..2] (counters).  This holds for every state reachable by
 *     inserts and by importing an exported state.
 *   - Lifetime.  A view that was never refreshed answers GNS_E_ARG.  A view is NOT
 *     staled by gns_ss_reset, gns_ss_reclaim, dictionary growth or
 *     gns_ss_import_state: it answers the refresh-point state until the next
 *     refresh.  Several views of one handle are independent.  Destroy views
 *     before their handle.
 *   - State capture.  regs, pbits, records or counters asked of a view whose last
 *     refresh did not carry GNS_SS_VIEW_STATE is GNS_E_ARG, before any device call.
 *     values and keys are always available.  Null output pointers are skipped.
 *   - Errors.  A null view, a null out (n > 0), a null n and stride < flow_bytes
 *     are GNS_E_ARG before any device call.  A cell whose key id named no
 *     dictionary slot at the refresh (corrupt state) is not dereferenced; the next
 *     reader call answers GNS_E_HIP.
 *   - A list call synchronizes the view's stream twice (the length, then the
 *     ordered rows) -- once more when the list outgrew its buffer, and once inside
 *     the order for keys longer than four bytes (its tie flag).
 * Memory: 4 + 4*ceil(flow_bytes/4) bytes per cell (depth*width); with state
 * another m + 8 bytes per cell, allocated at the first refresh that asks for it. */
typedef struct gns_ss_view gns_ss_view;
#define GNS_SS_VIEW_STATE 1u   /* refresh flag: also capture registers, pbits, counters, generator position */
int gns_ss_view_create(gns_ss *ss, gns_ss_view **out);
int gns_ss_view_destroy(gns_ss_view *v);
int gns_ss_view_refresh(gns_ss_view *v, uint32_t flags);
int gns_ss_view_query(gns_ss_view *v, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
int gns_ss_view_query_device(gns_ss_view *v, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
int gns_ss_view_heavy_hitters(gns_ss_view *v, uint8_t *flows, uint32_t *spreads, uint64_t *n);
int gns_ss_view_heavy_rows(gns_ss_view *v, uint8_t *rows_dev, uint64_t *n);
int gns_ss_view_export_state(gns_ss_view *v, uint32_t *values, uint8_t *keys, uint8_t *regs, double *pbits,
                             uint64_t *records, uint64_t *counters /* [3] */);

/* ------------------------------------------------------------------ */
/* Inputs: synthetic traffic and the pcap packer           */
/* ------------------------------------------------------------------ */
typedef struct gns_synth gns_synth;
typedef struct gns_synth_params {
    uint32_t flows;        /* flow universe F (default 2^20) */
    double zipf_s;         /* default 1.1 */
    uint64_t tuple_seed;   /* default 0x5EED0001 */
    uint64_t rank_seed;    /* default 0x5EED0002 */
    uint64_t len_seed;     /* default 0x5EED0003 */
    uint32_t shard, nshards; /* keep only flows whose src slot hashes to `shard` */
    int device;
    uint32_t fanout;       /* > 0: each packet's DstIP is drawn Zipf(zipf_s) over `fanout`
                              destinations instead of the flow's own (SuperSpread C3 shape) */
} gns_synth_params;
int gns_synth_create(const gns_synth_params *p, gns_synth **out);
int gns_synth_destroy(gns_synth *s);
/* Fill device buffers hdr[n*64], wirelen[n] with packets first..first+n-1 of
 * the (shard's) stream.  Deterministic, counter-based. */
int gns_synth_fill(gns_synth *s, uint8_t *hdr_dev, uint32_t *wirelen_dev, uint64_t first,
                   uint64_t n);
/* flow tuple of each shard-local flow (for tests): src16,dst16 [flows*16] etc */
int gns_synth_flows(gns_synth *s, uint32_t *n_flows);

/* capture file -> 64-byte records + wirelen (pkg/pcap/reader.go:35-49, which
 * opens it with libpcap's pcap_open_offline: classic pcap in either byte order
 * and time unit, or pcapng with any number of sections and interfaces;
 * Ethernet link type only).  Returns the number of records written (<= cap) or
 * a negative status; *total = packets in the file. */
int64_t gns_pack_pcap(const char *path, uint8_t *hdr, uint32_t *wirelen, uint64_t cap,
                      uint64_t *total);

/* as gns_pack_pcap, into compact records (see gns_cm_insert_compact): frames whose
 * tuple is not an IPv4 one go to side64 (side_cap records; *n_side = the number
 * written, or needed: GNS_E_RANGE when it exceeds side_cap) */
int64_t gns_pack_pcap_compact(const char *path, uint8_t *rec16, uint32_t *wirelen, uint64_t cap,
                              uint8_t *side64, uint64_t side_cap, uint64_t *n_side, uint64_t *total);
/* 64-byte records -> compact records on the device (all pointers DEVICE memory of
 * `device`; inputs complete before the call); *n_side as above */
int gns_compact_headers(const uint8_t *hdr, const uint32_t *wirelen, uint64_t n, uint8_t *rec16,
                        uint8_t *side64, uint64_t side_cap, uint64_t *n_side, int device);
/* the 16-byte forms (gns_cm_insert_compact with wirelen == NULL): GNS_E_RANGE when a
 * wire length exceeds 65535 */
int64_t gns_pack_pcap_compact16(const char *path, uint8_t *rec16, uint64_t cap, uint8_t *side64,
                                uint64_t side_cap, uint64_t *n_side, uint64_t *total);
int gns_compact_headers16(const uint8_t *hdr, const uint32_t *wirelen, uint64_t n, uint8_t *rec16,
                          uint8_t *side64, uint64_t side_cap, uint64_t *n_side, int device);
/* gns_pack_pcap_compact (wirelen == NULL: gns_pack_pcap_compact16) with the capture
 * timestamps gns_pack_pcap_ts writes: records, side array, counts and gns_pack_counts
 * are those of the call without timestamps (the exact aggregator's compact input) */
int64_t gns_pack_pcap_compact_ts(const char *path, uint8_t *rec16, uint32_t *wirelen, int64_t *ts_ns,
                                 uint64_t cap, uint8_t *side64, uint64_t side_cap, uint64_t *n_side,
                                 uint64_t *total);

/* [0] frames copied verbatim, [1] frames decoded on the host into 0x88B5
 * records, [2] frames without an IP layer, of the calling thread's last
 * gns_pack_pcap[_ts] call (records written only) */
int gns_pack_counts(uint64_t out[3]);

/* One captured frame -> one 64-byte record (what gns_pack_pcap writes for it):
 * a frame of the device fast-path shape (untagged IPv4, IHL 5, not a fragment,
 * TCP or non-tunnel UDP, by both caplen and wirelen) is copied verbatim;
 * any other frame is decoded here the way gopacket v1.1.19 + parser.go:23-67
 * decode it -- Ethernet/LLC/SNAP, any number of 802.1Q tags, IPv4 options,
 * IPv6 extension chains, IP-in-IP, GRE, VXLAN, Geneve, GTP-U, MPLS, PPPoE/PPP,
 * EtherIP; first IPv4 layer else first IPv6, first TCP layer else first UDP --
 * into a pre-parsed 0x88B5 record, or into a record the device drops when the
 * frame has no IP layer ("not an IP packet", parser.go:48-49).
 * Returns 0 verbatim, 1 decoded, 2 no IP layer, < 0 on a bad argument.
 * Replaces the per-packet gopacket.NewPacket decode of reader.go:35-49. */
int gns_frame_record(const uint8_t *frame, uint32_t caplen, uint32_t wirelen, uint8_t *rec64);

/* as gns_pack_pcap, plus ts_ns[n] = capture timestamp in ns (PacketInfo.Timestamp,
 * parser.go:30-33; gopacket opens captures with nanosecond precision) */
int64_t gns_pack_pcap_ts(const char *path, uint8_t *hdr, uint32_t *wirelen, int64_t *ts_ns, uint64_t cap,
                         uint64_t *total);

/* Thrift live path: decode n binary-protocol PacketInfo messages
 * (api/thrift/v1/traffic.thrift; packetcodec.go:97-108 UnmarshalPacketInfo over
 * apache/thrift v0.22.0) laid out back to back in buf, message i =
 * buf[offsets[i], offsets[i+1]), into DEVICE buffers hdr_out[n*64] (pre-parsed
 * 0x88B5 records), wirelen_out[n] = uint32(Length), ts_out[n] =
 * TimestampUnixNano.  A message the reference rejects becomes a record the
 * parser drops (*n_bad counts them).  buf/offsets live in `where`.  The records
 * feed gns_{cm,ss,ex}_insert_headers unchanged. */
int gns_thrift_decode(const uint8_t *buf, uint64_t buf_bytes, const uint64_t *offsets, uint64_t n,
                      uint8_t *hdr_out, uint32_t *wirelen_out, int64_t *ts_out, uint64_t *n_bad,
                      gns_mem where, int device);

/* ------------------------------------------------------------------ */
/* Flow routing for the multi-GPU path (BASELINE configs[3]) */
/* ------------------------------------------------------------------ */
/* Replaces the per-packet host split of the sharded deployment (SURVEY §8e:
 * "sharded by src-IP ... use the full key when SrcIP is not in the key";
 * go2netspectra_amd/dist.py owner_fields / owner_of_* are the host form).
 *
 * Every flow of every task must be owned by ONE shard, so that each shard's
 * sketch is exact for its sub-stream.  A router hashes an OWNER KEY made of
 * fields that every task's flow key contains (a flow key is the configured
 * fields, task.go:265-300; any non-empty field list is legal, config.go:59):
 * shard = mm3(owner key, 0xA5A5A5A5) % nshards.  IP slots enter the owner key
 * with an IPv4-mapped IPv6 slot folded to its IPv4 slot, so the owner is a
 * function of the EncodeFlow bytes and of the exact aggregator's To16 key alike.
 *
 * gns_route_owner_fields: the owner key of a set of tasks (a Manager's tasks,
 * manager.go:139-159 runs them on every packet): [SrcIP] when every task's key
 * holds SrcIP (configs[3]), else the fields common to all tasks in canonical
 * order (SrcIP, DstIP, SrcPort, DstPort, Protocol) -- for one task its whole
 * flow key.  GNS_E_ARG (with a message) when the tasks share no field: no
 * single owner exists for such a set.  Host logic only (no device needed). */
int gns_route_owner_fields(const gns_layout *tasks, uint32_t n_tasks, gns_layout *owner);
typedef struct gns_route gns_route;
/* nshards <= 64; owner = gns_route_owner_fields' result (or any non-empty field set) */
int gns_route_create_keyed(uint32_t nshards, const gns_layout *owner, int device, gns_route **out);
/* = gns_route_create_keyed with owner [SrcIP] */
int gns_route_create(uint32_t nshards, int device, gns_route **out);
int gns_route_destroy(gns_route *r);
int gns_route_owner_layout(gns_route *r, gns_layout *owner);
/* gns_route_partition reorders n DEVICE-resident 64-byte records (+ wire
 * lengths) into nshards runs, shard by shard, keeping packet order inside each
 * run (stable); counts[g] (host) = length of run g.  Records the parser drops
 * or does not support go to shard 0.  The call returns after the device work.
 * An all-to-all of run g to rank g, received runs concatenated in source-rank
 * order, delivers to every GPU exactly its stable filter of the stream. */
int gns_route_partition(gns_route *r, const uint8_t *hdr, const uint32_t *wirelen, uint64_t n,
                        uint8_t *out_hdr, uint32_t *out_wirelen, uint64_t *counts);
/* The same partition queued on `stream` (a hipStream_t; NULL = the router's own)
 * without waiting: counts_dev[g] (DEVICE int64) = length of run g once the stream
 * reaches it -- the all-to-all's split sizes stay on the device until the one
 * host read the exchange needs (dist.exchange_runs).  Partitions of one router
 * are ordered after each other whatever streams they are queued on (they share
 * its scratch). */
int gns_route_partition_async(gns_route *r, const uint8_t *hdr, const uint32_t *wirelen, uint64_t n,
                              uint8_t *out_hdr, uint32_t *out_wirelen, int64_t *counts_dev, void *stream);
/* Owner-routed queries (SURVEY §8e "queries are routed to the owner shard";
 * Sketch.Query, count_min.go:160-174 / super_spread.go:238-249, answers from the
 * shard that holds the flow): owner[i] = the shard owning flow key i, keys laid
 * out as key_layout (the querying task's FlowFields; it must contain every owner
 * field, else GNS_E_ARG).  keys and owner both in `where`; returns after the
 * device work.  dist.routed_query / the Go Router's QueryRouted exchange the
 * keys by owner, query each shard's handle and return the answers in order. */
int gns_route_owner_keys(gns_route *r, const gns_layout *key_layout, const uint8_t *keys, uint32_t stride,
                         uint64_t n, uint32_t *owner, gns_mem where);

/* ------------------------------------------------------------------ */
/* Exact aggregator (internal/engine/impl/exact/task.go)               */
/* ------------------------------------------------------------------ */
/* Replaces exact.New (task.go:83-103), Task.ProcessPacket (:124-149),
 * Task.Query (:298-326), Task.Snapshot (:153-191) and Task.Reset (:194-210).
 * Flows are keyed like the reference's string key strings.Join(fields, "-")
 * with IPs printed by net.IP.String(): the engine stores each IP field as its
 * 16-byte form (IPv4 and IPv4-mapped IPv6 -> ::ffff:a.b.c.d, other IPv6 as
 * is), which is equal exactly when the printed strings are equal. */
typedef struct gns_ex gns_ex;
typedef struct gns_ex_params {
    gns_layout key;          /* key_fields (task.go:330-366) */
    uint64_t max_flows;      /* initial flow dictionary capacity (default 4M; the table grows) */
    uint64_t batch_packets;  /* device batch (default 16M) */
    int device;
} gns_ex_params;
int gns_ex_create(const gns_ex_params *p, gns_ex **out);
int gns_ex_destroy(gns_ex *ex);
/* ProcessPacket over PacketInfo batches.  ipver[n]: 4 (net.IP of 4 bytes, IPv4
 * left-aligned in the 16-byte slots) or 6 (16-byte net.IP); ts_ns[n] =
 * PacketInfo.Timestamp.UnixNano(); t->length = ByteCount increment. */
int gns_ex_insert_tuples(gns_ex *ex, const gns_tuples *t, const uint8_t *ipver, const int64_t *ts_ns,
                         uint64_t n, gns_mem where);
/* fused parse of 64-byte records (as gns_cm_insert_headers) + timestamps */
int gns_ex_insert_headers(gns_ex *ex, const uint8_t *hdr, const uint32_t *wirelen, const int64_t *ts_ns,
                          uint64_t n, gns_mem where);
/* Compact records + timestamps, by the contract of gns_cm_insert_compact (see
 * gns_ss_insert_compact): equals gns_ex_insert_headers of the 64-byte records the
 * compact form was made from.  The IP versions of a tuple record are those of its
 * word 3 (IPv4 both ways in the 16-byte form), the ByteCount increment is the wire
 * length: 24 B/packet in the 16-byte form.  GNS_E_ARG also for a null ts_ns. */
int gns_ex_insert_compact(gns_ex *ex, const uint8_t *rec16, const uint32_t *wirelen, const int64_t *ts_ns,
                          uint64_t n, const uint8_t *side64, uint64_t n_side, gns_mem where);
int gns_ex_flush(gns_ex *ex);
/* out[i] = PacketCount << 32 | ByteCount (task.go:323); IP fields of the
 * encoded flow are read as 16-byte net.IPs, as the reference does; 0 if absent */
int gns_ex_query(gns_ex *ex, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
/* device keys / answers, as gns_cm_query_device */
int gns_ex_query_device(gns_ex *ex, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
/* Snapshot: *n_io = capacity in, number of flows out.  keys[n*key_bytes] in the
 * canonical 16-byte-IP layout; start/end = first/last packet timestamps
 * (stream order), pkts/bytes = PacketCount/ByteCount.  Any pointer may be NULL. */
int gns_ex_snapshot(gns_ex *ex, uint8_t *keys, int64_t *start_ns, int64_t *end_ns, uint64_t *pkts,
                    uint64_t *bytes, uint64_t *n_io);
/* Merge n rows of the form gns_ex_snapshot writes (canonical 16-byte-IP keys;
 * host or device pointers, device ones 8-byte aligned) into the table.  Each row
 * is one pseudo-record placed at the current end of the stream, row i after row
 * i-1, so timestamps follow the stream-order rule: a key not in the table is
 * created with the row's start and end; an existing key keeps its start and takes
 * the row's end; pkts and bytes add (u64 wrap).  Rows with pkts == 0 are ignored
 * (a flow exists iff it has packets).  The same key may occur in several rows.
 * A restore is a merge into an empty table; the union of two shards is a merge of
 * one's snapshot into the other.  gns_ex_counters changes only in [4] flows; the
 * table grows as for ingest; gns_ex_aggregate / gns_ex_heavy_hitters see merged
 * flows exactly as ingested ones. */
int gns_ex_merge(gns_ex *ex, const uint8_t *keys, const int64_t *start_ns, const int64_t *end_ns,
                 const uint64_t *pkts, const uint64_t *bytes, uint64_t n, gns_mem where);
/* Roll-up: re-key the flows of src onto dst's key layout, on the device.  The
 * reference answers a coarser question ("bytes per source address") with one task
 * per key layout, every task fed every packet (manager.go:232-244), or with GROUP BY
 * over stored rows (querier.go:251-319); here the coarser table is derived from the
 * resident one, after the traffic has arrived.
 *   - Layouts.  Every field of dst's layout must occur in src's; dst's fields may be
 *     fewer, equal or a permutation, in any order.  A field repeated in dst is copied
 *     once per occurrence, from src's first occurrence.  Keys stay in the canonical
 *     16-byte-IP form: the projection is a byte gather between the two layouts.
 *   - What it does.  Every flow gns_ex_snapshot(src) would list at the call (after
 *     src's pending batches) is projected onto dst's layout; the flows sharing one
 *     projected key form a group, and each group enters dst under the rule of
 *     gns_ex_merge as ONE pseudo-record: pkts and bytes are the group's sums (u64
 *     wrap), start is the start of the constituent whose first packet is earliest in
 *     src's stream, end the end of the one whose last packet is latest.  A key new to
 *     dst takes both; a key already in dst keeps its start, takes the group's end, and
 *     its counts add.  Consequence: a roll-up into an empty dst equals a handle of
 *     dst's layout fed the same inserts and merges as src, in keys, start, end, pkts
 *     and bytes -- with non-monotonic timestamps too, since start / end follow stream
 *     order, not min / max.  With equal layouts it is the device-to-device union of
 *     two shards.  (As in gns_ex_merge a flow exists iff it has packets: a group whose
 *     packet sum wraps to exactly 0 is not a flow.)
 *   - Positions.  src's stream positions are mapped behind dst's current stream end,
 *     and dst's position then advances by src's stream length (records inserted + rows
 *     merged since src was created): later inserts into dst come after every rolled-up
 *     flow, a dst view cursor taken before the call selects exactly the groups, and
 *     dst's per-flow positions stay exact, so dst can itself be a roll-up source.
 *   - out (may be NULL): [0] source flows projected, [1] flows new in dst.
 *   - Side effects.  src is read only: table, counters and cursors are unchanged.  Of
 *     dst's gns_ex_counters only [4] flows moves; dst grows as for gns_ex_merge.  The
 *     work runs in pieces of 2^20 source slots (GNS_EX_ROLLUP_PIECE in the
 *     environment, read at the call, sets another piece size: for tests only, so that
 *     small tables span many pieces); an error after the first piece (out of memory,
 *     a table at its 2^30-slot limit) leaves dst with the pieces merged so far.
 *   - Calling rules.  Synchronous, and an ingest-side call on BOTH handles: no other
 *     thread may insert into src or dst during it.  The device work is ordered after
 *     src's stream and runs on dst's.
 *   - GNS_E_ARG, dst untouched: a null handle (before any device call), dst == src, a
 *     field of dst that src's layout lacks, handles on different devices.  An empty
 *     src is GNS_OK and moves no flows.
 *   - Not offered: a view as source (view rows carry no stream positions, and adding
 *     them would change the views' documented memory); a delta roll-up ("since": rows
 *     are cumulative, so a delta is not additive).  (A distinct-flow count per group
 *     is gns_spread_rollup with src's whole key as the element layout.) */
int gns_ex_rollup(gns_ex *dst, gns_ex *src, uint64_t out[2]);
/* Prefix roll-up: gns_ex_rollup with the projected key's IP fields masked to a prefix --
 * "bytes per source /24", "which /16 is the flood coming from" -- on the device.
 *   - The mask applies to an IP field in the form the key stores it, the 16 bytes of
 *     net.IP.To16().  A value is IPv4 iff bytes 0..9 are zero and bytes 10, 11 are ff ff.
 *     An IPv4 value keeps bytes 0..11 and the leading *_v4 bits (0..32) of bytes 12..15;
 *     every other value keeps its leading *_v6 bits (0..128); the rest are zeroed.  Only
 *     trailing bits are cleared, so no value changes class, the mask is idempotent, and a
 *     coarser mask over a finer one is the coarser one (coarser in both classes).  v4 = 0
 *     sends every IPv4 address to ::ffff:0.0.0.0, v6 = 0 every other address to ::.
 *     Ports and protocol are never masked.
 *   - Everything else is gns_ex_rollup's: layouts, one pseudo-record per group under the
 *     rule of gns_ex_merge, start / end in stream order, positions mapped behind dst's
 *     stream end, out, pieces (GNS_EX_ROLLUP_PIECE), calling rules.  Consequence: into an
 *     empty dst the result equals a handle of dst's layout fed src's packets WITH THEIR
 *     ADDRESSES MASKED, in keys, start, end, pkts and bytes.  With {32,128,32,128} it
 *     equals gns_ex_rollup bit for bit.  A prefix for a field dst's layout lacks is ignored.
 *   - dst is a full handle, and can be the source of a coarser prefix roll-up:
 *     /24 -> /16 -> /8 chained equals each rolled up directly from the flow table.
 *   - GNS_E_ARG, dst untouched: gns_ex_rollup's cases; px == NULL, *_v4 > 32 or
 *     *_v6 > 128 (after the null-handle check and before any device call). */
typedef struct gns_prefix { uint8_t src_v4, src_v6, dst_v4, dst_v6; } gns_prefix;   /* bits kept; {32,128,32,128} keeps all */
int gns_ex_rollup_prefix(gns_ex *dst, gns_ex *src, const gns_prefix *px, uint64_t out[2]);
int gns_ex_reset(gns_ex *ex);
/* out[8]: inserted, dropped, unsupported, dictionary full, flows, records, batches, 0 */
int gns_ex_counters(gns_ex *ex, uint64_t out[8]);
/* [0] table growths, [1] 0, [2] slots, [3] claimed slots, [4] growth time (us),
 * [5] batches re-run after a dictionary overflow, [6] slots, [7] growths */
int gns_ex_dict_stats(gns_ex *ex, uint64_t out[8]);
int gns_ex_set_timing(gns_ex *ex, int on);
/* stages: 0 extract, 1 resolve, 2 partition, 3 aggregate, 4 hot flows + timestamps, 5 total
 * (of an insert batch), 6 query (the device work of gns_ex_aggregate / gns_ex_heavy_hitters),
 * 7 view (the device work of gns_ex_view_refresh) */
int gns_ex_stage_times(gns_ex *ex, double ms[8], uint64_t launches[8], int reset);

/* Query plane: the three questions of query.Querier (internal/query/querier.go)
 * answered from the live flow table instead of ClickHouse.  Both calls are
 * ordered after pending insert batches exactly as gns_ex_snapshot is, and see
 * exactly the flows gns_ex_snapshot lists.
 *
 * A filter is appendAggregationFilters / appendTraceFlowFilters
 * (querier.go:143-188): equality on the masked fields, AND-ed.  A masked field
 * that is not part of the handle's key layout matches no flow: the reference
 * stores such a column as NULL (getNullableField, exact/writer_clickhouse.go:142-148)
 * and `NULL = ?` selects nothing.  mask == 0 matches every flow: the totals of
 * AlerterMsg (exact/task.go:224-233). */
typedef struct gns_ex_filter {
    uint32_t mask;        /* OR of (1u << gns_field): that field must equal the value below */
    uint8_t  src16[16];   /* net.IP.To16() form: IPv4 as ::ffff:a.b.c.d, the form keys are stored in */
    uint8_t  dst16[16];
    uint16_t sport, dport;  /* host order */
    uint8_t  proto, _pad[3];
} gns_ex_filter;
/* AggregateFlows' row (querier.go:251-319) and TraceFlow's (querier.go:322-372) in one */
typedef struct gns_ex_summary {
    uint64_t flows, packets, bytes;     /* COUNT(*), SUM(PacketCount), SUM(ByteCount), mod 2^64 */
    int64_t  first_ns, last_ns;         /* min(StartTime), max(EndTime), signed; 0, 0 when flows == 0 */
    uint64_t max_packets, max_bytes;    /* TraceFlow's max(PacketCount), max(ByteCount); 0 when flows == 0 */
} gns_ex_summary;
/* out[i] = the summary of the flows matching filters[i] (host arrays).  One pass
 * over the table answers 64 filters; a longer batch takes ceil(nf / 64) passes.
 * nf == 0 is a no-op.  GNS_E_ARG: a null pointer, mask bits outside the five fields. */
int gns_ex_aggregate(gns_ex *ex, const gns_ex_filter *filters, uint32_t nf, gns_ex_summary *out /* [nf] */);
/* CIDR filters: a gns_ex_filter whose masked SrcIP / DstIP must match only in their leading
 * src_bits / dst_bits bits of the 16-byte To16 form -- an IPv4 /24 is 96 + 24 = 120, 128 is
 * gns_ex_filter's equality, 0 matches every flow whose key has the field.  Bits of the
 * filter's address below the prefix are ignored.  The bits of a field the mask leaves open
 * mean nothing.  Everything else is gns_ex_aggregate's (a masked field outside the handle's
 * layout matches nothing; 64 filters per pass); GNS_E_ARG also for bits above 128. */
typedef struct gns_ex_cidr { gns_ex_filter f; uint8_t src_bits, dst_bits, _pad[2]; } gns_ex_cidr;  /* bits of the To16 form, 0..128 */
int gns_ex_aggregate_cidr(gns_ex *ex, const gns_ex_cidr *filters, uint32_t nf, gns_ex_summary *out /* [nf] */);
/* QueryHeavyHitters ... ORDER BY LatestValue DESC LIMIT ? (querier.go:191-248), and the
 * truth side of Count-Min's heavy hitters (cm_test.go:124-137).
 * metric 0: PacketCount, 1: ByteCount.  Flows with value >= threshold, in the canonical list order
 * (value descending, key bytes ascending), cut to the first `limit` rows when limit != 0.
 * *n_io: capacity in, list length (after the cut) out; a list longer than the capacity is
 * reported and not written (as gns_exs_heavy_hitters).  keys[n*key_bytes] in the layout of
 * gns_ex_snapshot, values 64-bit.  threshold 0 lists every flow.  keys / values may be NULL. */
int gns_ex_heavy_hitters(gns_ex *ex, int metric, uint64_t threshold, uint64_t limit,
                         uint8_t *keys, uint64_t *values, uint64_t *n_io);
/* The signed heavy changers of a table whose counts are changes (gns_ex_hist_rollup_between):
 * v = the packet (metric 0) or byte (metric 1) word read as int64.  A group is listed when it
 * is a flow (pkts != 0), v != 0, the sign of v matches direction (+1: increases, -1: decreases,
 * 0: either) and |v| >= max(threshold, 1), |v| as u64 (INT64_MIN has magnitude 2^63).  Order:
 * |v| descending, key bytes ascending, cut to `limit` rows when limit != 0; values[] holds v
 * itself.  *n_io, keys, values as gns_ex_heavy_hitters; GNS_E_ARG also for another direction. */
int gns_ex_movers(gns_ex *ex, int metric, int direction, uint64_t threshold, uint64_t limit,
                  uint8_t *keys, int64_t *values, uint64_t *n_io);

/* Snapshot view: the table, or the flows touched since a cursor, exported and queried
 * CONCURRENTLY with ingest.  The reference's snapshotter hands every flow of every exact
 * task to a writer each interval while the workers keep inserting (manager.go:139-159,
 * exact/task.go:154-194), and the alerter reads the totals (exact/task.go:224-233).  A view
 * holds a dense copy of the selected flows, key bytes included, so it stays valid
 * whatever the handle does afterwards: insert, merge, table growth, reset.
 *   - Refresh point.  gns_ex_view_refresh is an ingest-side call (serialised with the
 *     handle's other calls) and asynchronous on the handle's stream.  The view then answers
 *     for the state after every insert or merge issued before that refresh, whatever
 *     follows on the handle.  A reset does not stale it (unlike a Count-Min view): nothing
 *     is resolved through the live dictionary.
 *   - since == 0 selects every flow gns_ex_snapshot would list at that point.  since == a
 *     cursor an earlier refresh of this handle returned selects only the flows that took a
 *     packet or a merged row after that point.  since beyond the current position:
 *     GNS_E_ARG, the view is untouched.
 *   - Cursor.  *cursor = the next stream position the handle will assign (records inserted
 *     + rows merged so far; positions never restart): feed it to the next refresh.  A
 *     cursor taken before gns_ex_reset selects every flow of the new period, since the
 *     table was emptied after it.  cursor may be NULL.
 *   - Rows carry cumulative state (start, end, pkts, bytes as of the refresh), not
 *     increments, in dictionary-slot order: gns_ex_view_snapshot after a refresh with
 *     since == 0 returns arrays bit-equal to gns_ex_snapshot called at that point.  The
 *     reference's store keeps the latest row per flow (argMax(..., Timestamp),
 *     querier.go:191-248), so a writer that stores only each interval's delta answers
 *     every query as one that stores the whole table each time.
 *   - gns_ex_view_snapshot / _aggregate / _heavy_hitters take the arguments of
 *     gns_ex_snapshot / gns_ex_aggregate / gns_ex_heavy_hitters and answer over the view's
 *     rows.  They may run on any thread while the handle ingests, on the view's own
 *     stream, and allocate and free nothing once warm.  There is no point query: a filter
 *     on every key field through gns_ex_view_aggregate is one (TraceFlow).
 *   - A view that was never refreshed answers GNS_E_ARG.  A refresh waits for a reader
 *     call in progress on the same view.  Null-argument checks run before any device
 *     call.  Destroy a view before its handle.
 * Memory: a record plus 32 bytes per row, for the flows the handle held at the refresh
 * (the buffers only grow), and 8 MB of pinned host staging. */
typedef struct gns_ex_view gns_ex_view;
int gns_ex_view_create(gns_ex *ex, gns_ex_view **out);
int gns_ex_view_destroy(gns_ex_view *v);
int gns_ex_view_refresh(gns_ex_view *v, uint64_t since, uint64_t *cursor);
int gns_ex_view_snapshot(gns_ex_view *v, uint8_t *keys, int64_t *start_ns, int64_t *end_ns,
                         uint64_t *pkts, uint64_t *bytes, uint64_t *n_io);
int gns_ex_view_aggregate(gns_ex_view *v, const gns_ex_filter *f, uint32_t nf, gns_ex_summary *out);
/* gns_ex_aggregate_cidr over the view's rows, under the rules of gns_ex_view_aggregate */
int gns_ex_view_aggregate_cidr(gns_ex_view *v, const gns_ex_cidr *f, uint32_t nf, gns_ex_summary *out);
int gns_ex_view_heavy_hitters(gns_ex_view *v, int metric, uint64_t threshold, uint64_t limit,
                              uint8_t *keys, uint64_t *values, uint64_t *n_io);

/* History: the store behind the Querier's EndTime.  Every request of query.Querier carries
 * an EndTime and each query adds `Timestamp <= ?` on the snapshot time (querier.go:211-213,
 * 271-273, 344-346); the reference answers from the per-interval snapshot rows its writer
 * stored under one Timestamp (manager.go:139-159).  A history is that store on the device: an
 * append-only log of the rows of refreshed views, each append one snapshot.
 *   - Snapshots 0..S-1 carry strictly increasing timestamps (int64 ns, negative values are
 *     legal).  gns_ex_hist_append adds the rows of one refreshed gns_ex_view -- whole
 *     (since == 0) or a delta, the store answers the same either way -- as snapshot S.  It is
 *     a reader call on the view: a concurrent refresh of the view waits, the handle keeps
 *     ingesting, and the call may run on the snapshotter's thread.  out[0] = rows appended,
 *     out[1] = keys new to the history (out may be NULL).  A view without rows is legal and
 *     registers the timestamp.
 *   - A query names a time by end_ns: NULL is the newest snapshot, else s(T) = the newest
 *     snapshot with timestamp <= *end_ns; with none the query answers as an empty table.  A
 *     row written by snapshot a is SEEN when a <= s(T) and LIVE when no later row of the same
 *     key is seen too: the argMax(..., Timestamp) of the reference.  The store never forgets
 *     a flow by itself (only gns_ex_hist_trim removes rows): rows written before a
 *     gns_ex_reset of the source handle stay, and a flow that comes back after it supersedes
 *     its old row with its new, smaller counts.
 *   - gns_ex_hist_aggregate[_cidr] take the filters of gns_ex_aggregate[_cidr] unchanged (a
 *     masked field outside the layout matches nothing).  flows, packets, bytes are COUNT / SUM
 *     over the matching LIVE rows (AggregateFlows); first_ns, last_ns, max_packets, max_bytes
 *     are min / max over the matching SEEN rows, superseded ones included (TraceFlow has no
 *     argMax); all zero when no seen row matches.  A history holding one whole view answers
 *     bit-equal to gns_ex_view_aggregate of that view.
 *   - gns_ex_hist_heavy_hitters lists the LIVE rows under the rules and the *n_io protocol of
 *     gns_ex_heavy_hitters.  gns_ex_hist_snapshot returns the LIVE rows in log order
 *     (snapshot, then the view's row order) under the protocol of gns_ex_snapshot.
 *   - gns_ex_hist_times: *n_io capacity in, the number of snapshots out; ts may be NULL.
 *     gns_ex_hist_stats: snapshots, rows, distinct keys, row capacity, index slots, index
 *     growths, log growths, rows released by trims (cumulative).
 *   - gns_ex_hist_trim expires the c snapshots with timestamp < before_ns, a prefix of the log.
 *     fold == 0 drops them with all their rows (the reference's DROP PARTITION): the history
 *     then equals one to which only the later snapshots were ever appended, a flow whose
 *     every row expired is forgotten (appended again it counts as a new key), and with every
 *     snapshot expired the history is empty.  fold == 1 folds them into one base snapshot:
 *     of their rows those LIVE as of the last expired snapshot stay, in log order, as
 *     snapshot 0 under that snapshot's timestamp, followed by the later snapshots unchanged;
 *     every aggregate, heavy-hitter and snapshot answer with end time at or after that
 *     timestamp is unchanged, earlier end times answer as an empty table, and the min / max
 *     members of a summary (taken over SEEN rows) range over the rows that remain.  Nothing
 *     expired (c == 0), or fold with c == 1, is a no-op that moves and allocates nothing.
 *     out[0] = snapshots removed (fold: c - 1, the base replaces them), out[1] = rows
 *     released, out[2] = keys forgotten, out[3] = rows now held (out may be NULL).  The kept
 *     rows move into a new log sized for them and the key index is rebuilt (smaller when keys
 *     were forgotten); the new state is published last, so on any failure the history is
 *     untouched.  Queries from other threads wait for the trim and then see the trimmed store.
 *   - gns_ex_hist_export writes every log row in log order under the *n_io protocol of
 *     gns_ex_snapshot: canonical key bytes, start, end, pkts, bytes and the number of the
 *     snapshot that wrote the row (any array may be NULL); timestamps come from
 *     gns_ex_hist_times.  gns_ex_hist_append_rows appends one snapshot from host arrays of that
 *     form, as gns_ex_hist_append does from a view (n == 0 registers the timestamp); feeding
 *     an empty history the exported rows snapshot by snapshot restores it.  GNS_E_ARG with
 *     every answer unchanged: a row without packets, and two rows of one call with the same
 *     key (found on the device before anything is linked; the key index may have grown).
 *   - max_rows / max_flows are only the INITIAL capacities of the log and of the key index
 *     (0: 2^20 rows, 2^16 keys); both grow.  GNS_E_FULL is left only for a log beyond
 *     2^32 - 2 rows or snapshots (and the dictionary's 2^30 slots).
 *   - GNS_E_ARG with the history untouched, checked before any device call: a null handle, a
 *     view that was never refreshed, a view whose handle's key layout differs from the
 *     history's, a view on another device, timestamp_ns <= the last snapshot's, a trim's
 *     fold outside {0, 1}, and the filter / metric errors of the live calls.  Nothing of a snapshot is visible to a query
 *     before its append has returned GNS_OK.
 *   - Threads: any, serialised by the history's mutex; its stream and pinned staging are its
 *     own and no query allocates or frees once warm.  A history does not refer to the
 *     handle or the view after the append returns: either may be destroyed first.
 * Memory: a record plus 40 bytes per log row (32 of state, 8 of version words); per index
 * slot a record plus 4 bytes; 8 MB of pinned host staging.  A trim builds the new log beside
 * the old one (blocks of one launch would otherwise read rows that others had overwritten):
 * its peak is the old log plus the new, plus 4 bytes per expired row under fold and a second
 * index while keys are forgotten; the old log is freed when the trim returns.
 * gns_ex_hist_append_rows stages the call's key rows on the device.  (The sketch tasks'
 * heavy-hitter lists have a history of their own: gns_hh_hist_*, below.)
 *
 * gns_ex_hist_rollup: the table as of end_ns re-keyed into dst, on the device -- the GROUP BY
 * the reference would run over its stored rows (querier.go:251-372).  The source is the LIVE
 * rows as of s(T), the rows gns_ex_hist_snapshot lists (none when no snapshot lies at or
 * before *end_ns: GNS_OK, nothing moves); each is projected onto dst's layout, under px
 * masked to a prefix, and merged into dst group by group:
 *   - pkts / bytes: the sums over the group (u64 wrap).  A group whose packet sum wraps to
 *     exactly 0 is not a flow, as in gns_ex_merge and gns_ex_rollup.
 *   - start = min(StartTime), end = max(EndTime), both signed.  NOT the stream-order rule of
 *     gns_ex_rollup: log rows carry no stream positions, and min / max is what TraceFlow and
 *     AggregateFlows compute over stored rows, whatever the order of rows inside a snapshot.
 *   - A key already in dst: counts add, start becomes the smaller and end the larger of the
 *     two.  Two shards' histories rolled into one dst are their union, in either order.
 *   - Positions: log row r enters dst at stream position B + r, B = dst's stream end at the
 *     call; a group's first / last are the min / max of those, and dst's position advances
 *     by the rows as of s(T).  As after gns_ex_rollup, later inserts come after every rolled-up
 *     flow, a view cursor taken before the call selects exactly the groups, and dst is a full
 *     handle: a source for gns_ex_rollup[_prefix] and gns_spread_rollup, views, queries, merge.
 *   - Limit: a further gns_ex_rollup of such a table applies THAT call's stream-order rule
 *     over these positions, so a chain keeps counts exact but keeps min / max times only for
 *     timestamps monotone in the log.  Roll each level from the history when the times matter.
 *   - Layouts as gns_ex_rollup: dst's fields may be fewer than the history's, equal to them, a
 *     permutation of them, or repeated.  Prefixes as gns_ex_rollup_prefix (px == NULL: unmasked):
 *     the class test runs on the unmasked bytes, a prefix for a field dst lacks is ignored.
 *   - out (may be NULL): out[0] = live rows projected, out[1] = flows new in dst.
 *   - GNS_E_ARG with dst untouched, checked before any device call: a null handle, a dst field
 *     outside the history's layout (named in the error text), different devices, a prefix out
 *     of range.
 *   - Calling rules: a reader call on the history -- its mutex is held until dst's stream has
 *     drained, so a concurrent trim cannot free the log under the kernels and a concurrent
 *     append waits -- and an ingest-side call on dst.  The device work runs on dst's stream,
 *     ordered after the history's, in pieces of 2^20 log rows.  An error after the first piece
 *     leaves the pieces merged so far; the positions are spent.
 *
 * gns_ex_hist_rollup_between: what changed between two times, re-keyed into dst on the device.
 * s0 = s(*start_ns) (-1 for NULL and before the first snapshot), s1 = s(*end_ns) (NULL: the
 * newest).  A log row with version words (a, b) = (written, superseded) is a PLUS row when
 * s0 < a <= s1 < b (live at T1, stored in the window), a MINUS row when a <= s0 < b <= s1 (live
 * at T0, displaced in the window) and takes no part otherwise -- the row live at both times,
 * the common one, is never loaded: rows are in snapshot order, so the rows below those as of
 * s0 can only be minus rows and the rows from there to those as of s1 only plus rows, one
 * version word per row decides, and nothing beyond is scanned.  Selected rows are projected
 * (under px masked) and merged per projected key as in gns_ex_hist_rollup, with
 *   - pkts / bytes: plus rows add, minus rows subtract (u64 wrap): the stored words are the
 *     two's-complement signed change sum v(T1) - sum v(T0); read them as int64.  A group whose
 *     packet change is exactly 0 is not a flow (the rule above), so its byte change is NOT
 *     reported even when it is not 0.
 *   - start = min(StartTime), end = max(EndTime) over the group's PLUS rows: the times of the
 *     rows stored in the window and still current at T1.  Minus rows take no part; the store
 *     has no tombstones, so every key with a minus row has a plus row.  A history stored as
 *     whole views (not deltas) stores a row per flow and snapshot, so an unchanged flow yields
 *     a plus and a minus row of equal counts: they cancel in the counts and the plus row widens
 *     a coarser group's times.
 *   - A key already in dst, positions (dst advances by the rows as of s1 when the scan runs),
 *     layouts, prefixes, calling rules, pieces and error behaviour: gns_ex_hist_rollup's.  When
 *     s1 < 0 or s0 == s1 nothing is scanned, no position is spent and out = {0, 0}.
 *   - s0 = -1: gns_ex_hist_rollup(dst, h, end_ns, px), bit for bit.
 *   - out (may be NULL): out[0] = rows selected (plus + minus), out[1] = slots claimed in dst:
 *     the projected keys new to it, those of groups whose packet change is 0 included.
 *   - Such a no-flow group keeps its slot, byte change and times while window calls follow one
 *     another into dst (table growth inside this call moves every slot a row has reached), and
 *     loses them at the next growth of dst in any other call (insert, merge, the as-of roll-up):
 *     what a later row of that key adds to is history-dependent.  Do not rely on it.
 *   - GNS_E_ARG before any device call also for *start_ns > *end_ns (both given).
 * There is no counter-reset rule: a flow that came back smaller after a reset of the task
 * reports a negative change, the honest table(T1) - table(T0).  gns_ex_movers (above) lists the
 * heavy changers of such a table.
 * Not offered: a spread table straight from the log (go through a same-layout roll-up and
 * gns_spread_rollup), movers on views or straight off the log. */
typedef struct gns_ex_hist gns_ex_hist;
typedef struct gns_ex_hist_params { gns_layout key; uint64_t max_rows, max_flows; int device; } gns_ex_hist_params;
int gns_ex_hist_create(const gns_ex_hist_params *p, gns_ex_hist **out);
int gns_ex_hist_destroy(gns_ex_hist *h);
int gns_ex_hist_append(gns_ex_hist *h, gns_ex_view *v, int64_t timestamp_ns, uint64_t out[2]);
int gns_ex_hist_append_rows(gns_ex_hist *h, const uint8_t *keys, const int64_t *start_ns, const int64_t *end_ns,
                            const uint64_t *pkts, const uint64_t *bytes, uint64_t n, int64_t timestamp_ns,
                            uint64_t out[2]);
int gns_ex_hist_trim(gns_ex_hist *h, int64_t before_ns, int fold, uint64_t out[4]);
int gns_ex_hist_export(gns_ex_hist *h, uint8_t *keys, int64_t *start_ns, int64_t *end_ns, uint64_t *pkts,
                       uint64_t *bytes, uint32_t *written, uint64_t *n_io);
int gns_ex_hist_times(gns_ex_hist *h, int64_t *ts, uint64_t *n_io);
int gns_ex_hist_stats(gns_ex_hist *h, uint64_t out[8]);
int gns_ex_hist_aggregate(gns_ex_hist *h, const int64_t *end_ns, const gns_ex_filter *f, uint32_t nf, gns_ex_summary *out);
int gns_ex_hist_aggregate_cidr(gns_ex_hist *h, const int64_t *end_ns, const gns_ex_cidr *f, uint32_t nf, gns_ex_summary *out);
int gns_ex_hist_heavy_hitters(gns_ex_hist *h, const int64_t *end_ns, int metric, uint64_t threshold, uint64_t limit,
                              uint8_t *keys, uint64_t *values, uint64_t *n_io);
int gns_ex_hist_snapshot(gns_ex_hist *h, const int64_t *end_ns, uint8_t *keys, int64_t *start_ns, int64_t *end_out_ns,
                         uint64_t *pkts, uint64_t *bytes, uint64_t *n_io);
int gns_ex_hist_rollup(gns_ex *dst, gns_ex_hist *h, const int64_t *end_ns, const gns_prefix *px, uint64_t out[2]);
int gns_ex_hist_rollup_between(gns_ex *dst, gns_ex_hist *h, const int64_t *start_ns, const int64_t *end_ns,
                               const gns_prefix *px, uint64_t out[2]);

/* ------------------------------------------------------------------ */
/* Heavy-hitter history: QueryHeavyHitters' EndTime for the sketches   */
/* ------------------------------------------------------------------ */
/* QueryHeavyHitters (internal/query/querier.go:191-248) reads the heavy_hitters table, which only
 * the sketch tasks write: one row (Timestamp, TaskName, Flow, Value, Type) per list entry of each
 * interval's Snapshot() (internal/engine/impl/sketch/writer_clickhouse.go:86-138; Type 0 =
 * Count-Min's count list, 1 = its size list, 2 = SuperSpread's list).  The query is
 *   SELECT Flow, argMax(Value, Timestamp) ... WHERE TaskName = ? AND Type = ? [AND Timestamp <= ?]
 *   GROUP BY Flow ORDER BY LatestValue DESC LIMIT ?
 * A gns_hh_hist is that table on the device for one task (TaskName is fixed) and one flow width
 * key_bytes (1..37): a log per Type 0..255 over one key index, append-only but for gns_hh_hist_trim; the types are
 * independent tables that share the snapshot timestamps.
 *   - Snapshots 0..S-1 carry STRICTLY increasing timestamps (int64 ns, negative values are
 *     legal).  The reference's DateTime has second resolution and two snapshots within one second
 *     tie in argMax; requiring strictly increasing timestamps is the defined behaviour here.  One
 *     gns_hh_hist_append is one snapshot: zero or more lists of packed rows [flow (key_bytes) |
 *     u32 LE value] -- the rows gns_cm_heavy_rows, gns_cm_view_heavy_rows and
 *     gns_ss_view_heavy_rows give -- each under its type, at most one list per type.  `where`
 *     names the memory of every list's rows: device memory of the history's GPU (no copy of the
 *     list passes through the host), or host memory (staged to the device, then the same path: a
 *     restore).  An append without rows registers its timestamp.  out[0] = rows appended,
 *     out[1] = (type, flow) pairs new to the history (out may be NULL).
 *   - A query names a time by end_ns: NULL is the newest snapshot, else s(T) = the newest
 *     snapshot with timestamp <= *end_ns; with none every answer is empty.  For a type, a row is
 *     SEEN when its snapshot is <= s(T) and LIVE when no later SEEN row of the same (type, flow)
 *     exists.  There are NO TOMBSTONES: a flow that was listed once and is missing from every
 *     later list stays LIVE with its last listed value (argMax only sees rows that exist), and a
 *     flow listed again supersedes its old row even with a smaller value (the normal case after
 *     the sketch's Reset).  GROUP BY Flow groups by the decoded string; DecodeFlow is injective on
 *     the key bytes of a fixed layout, so the grouping is by key bytes.
 *   - gns_hh_hist_heavy_hitters lists the LIVE rows of one type with value >= threshold, value
 *     descending, then flow bytes ascending (ClickHouse leaves ties unordered: this is the
 *     canonical list order of gns_ex_heavy_hitters), cut to `limit` rows when limit != 0, under
 *     the *n_io protocol of gns_ex_heavy_hitters (capacity in, list length after the cut out; a
 *     longer list is reported and not written; flows / values may be NULL).  Values are u32 in
 *     the log, as every producer emits them, and 64-bit in the answer; value 0 is a legal row.  A
 *     type that was never appended answers empty.  gns_hh_hist_heavy_rows gives the same list as
 *     packed device rows (capacity *n_io rows of key_bytes + 4), e.g. for gns_hh_order_rows after
 *     an all-gather of several GPUs' flow-disjoint histories.
 *   - Rows of one list must name distinct flows (the engines' lists do).  They are caller memory
 *     all the same, so the device checks every list before anything is linked.
 *   - A rejected append leaves every answer, gns_hh_hist_times and the first three stats
 *     unchanged (the key index may have grown).  GNS_E_ARG: a null handle, two rows of a list with
 *     the same flow, two lists of one type, a type above 255, timestamp_ns <= the last
 *     snapshot's, rows that are not device memory of the history's GPU.  GNS_E_FULL: a type's
 *     log beyond 2^32 - 2 rows, 2^32 - 2 snapshots, the index beyond 2^30 slots.  All lists of a
 *     snapshot are resolved and checked before any is linked, and nothing of a snapshot is
 *     visible to a query before its append has returned GNS_OK.
 *   - gns_hh_hist_times: as gns_ex_hist_times.  gns_hh_hist_stats: snapshots, rows, distinct
 *     (type, flow) pairs, lanes (types that hold rows or had a lane made for them), row capacity
 *     (all lanes), index slots, index growths, log growths.
 *   - gns_hh_hist_export writes every log row in (type, log order) -- type, flow bytes, value,
 *     the number of the snapshot that wrote the row; any array may be NULL -- under the *n_io
 *     protocol of gns_ex_hist_export; timestamps come from gns_hh_hist_times.  Feeding an empty
 *     history each snapshot's rows, as host lists, restores it.
 *   - max_rows / max_flows are only the INITIAL capacities of a type's log and of the key index
 *     (0: 2^20 rows, 2^16 flows); both grow.
 *   - Threads: any, serialised by the history's mutex; its stream and pinned staging are its own
 *     and no query allocates or frees once warm.  The history keeps no reference to the
 *     caller's rows, handle or view after the append returns.
 *   - gns_hh_hist_trim expires the c snapshots with timestamp < before_ns: in every lane a prefix
 *     of the log, the rows of snapshots 0..c-1 (none for a type first appended later).  out[0] =
 *     snapshots removed, out[1] = rows removed over all lanes, out[2] = (type, flow) pairs
 *     forgotten, out[3] = rows left (out may be NULL).
 *       fold = 0 (drop): the snapshots and their rows are gone, as a dropped partition of the
 *         reference's table (PARTITION BY toYYYYMM(Timestamp), writer_clickhouse.go:25-27): every
 *         answer at every T is what the SQL gives over the table without the rows with
 *         Timestamp < before_ns.  A (type, flow) pair whose newest row expired is forgotten (it
 *         counts as new when appended again), a key no type names any more leaves the index, and
 *         the index is rebuilt to the size of what is left.  A type that loses every row keeps
 *         its lane: it answers empty and takes later appends.
 *       fold = 1: the expired snapshots become ONE base snapshot under the timestamp of snapshot
 *         c - 1, holding per type the expired rows that are live as of it, written = 0.  Every
 *         answer at T >= that timestamp is unchanged, every answer below it is empty, and no pair
 *         and no key is forgotten.  Because the store has no tombstones a fold keeps one row per
 *         pair ever listed: it bounds the log by (snapshots kept) x (list length) + (distinct
 *         pairs), and it never shrinks the index.  Only drop bounds the index.
 *     c == 0, and c == 1 under fold (the base is snapshot 0 itself), change nothing and return
 *     GNS_OK with out = {0, 0, 0, rows}.  The kept rows move stably into a new, smaller log per
 *     type (log order stays snapshot order) and the snapshot numbers in them lose what was
 *     removed; the new logs, head words and index are built beside the live ones and published
 *     last, so a trim that fails leaves every answer, gns_hh_hist_times, _stats and _export as
 *     they were.  The old logs are freed before the call returns.  GNS_E_ARG: a null handle, a
 *     fold other than 0 / 1.
 *   - gns_hh_hist_query answers a batch of n flows (key_bytes each; host memory, or device memory
 *     of the history's GPU, as `where` says of flows, values and found alike) with the value of the
 *     LIVE row of (type, flow) as of s(T): values[i] (u64) and found[i] = 1.  A flow without a
 *     live row -- never listed, listed only later, forgotten by a drop, a type never appended, T
 *     before the first snapshot -- answers found = 0, value = 0 (value 0 is a legal row, hence
 *     found).  A flow named several times is answered each time; n == 0 is legal.  The call
 *     never inserts into the index: gns_hh_hist_stats is the same after any number of queries.
 *     As of the newest snapshot it reads head words; as of an older one it makes one pass over
 *     the rows of snapshots 0..s(T) of that type, the cost class of gns_hh_hist_heavy_hitters
 *     without a limit.
 * Memory: 16 bytes per log row (key bytes live only in the index); per index slot a record plus
 * 4 bytes per type in use; 8 MB of pinned host staging.
 * Not offered: roll-ups. */
typedef struct gns_hh_hist gns_hh_hist;
typedef struct gns_hh_hist_params { uint32_t key_bytes; uint64_t max_rows, max_flows; int device; } gns_hh_hist_params;
typedef struct gns_hh_list { uint32_t type; const uint8_t *rows; uint64_t n; } gns_hh_list;   /* packed [flow | u32 LE value] */
int gns_hh_hist_create(const gns_hh_hist_params *p, gns_hh_hist **out);
int gns_hh_hist_destroy(gns_hh_hist *h);
int gns_hh_hist_append(gns_hh_hist *h, int64_t timestamp_ns, const gns_hh_list *lists, uint32_t nlists, gns_mem where,
                       uint64_t out[2]);
int gns_hh_hist_heavy_hitters(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, uint64_t threshold, uint64_t limit,
                              uint8_t *flows, uint64_t *values, uint64_t *n_io);
int gns_hh_hist_heavy_rows(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, uint64_t threshold, uint64_t limit,
                           uint8_t *rows_dev, uint64_t *n_io);
int gns_hh_hist_times(gns_hh_hist *h, int64_t *ts, uint64_t *n_io);
int gns_hh_hist_stats(gns_hh_hist *h, uint64_t out[8]);
int gns_hh_hist_export(gns_hh_hist *h, uint8_t *types, uint8_t *flows, uint32_t *values, uint32_t *written,
                       uint64_t *n_io);
int gns_hh_hist_trim(gns_hh_hist *h, int64_t before_ns, int fold, uint64_t out[4]);
int gns_hh_hist_query(gns_hh_hist *h, const int64_t *end_ns, uint32_t type, const uint8_t *flows, uint64_t n, gns_mem where,
                      uint64_t *values, uint8_t *found);

/* ------------------------------------------------------------------ */
/* Exact spread: the device ground truth of SuperSpread                */
/* ------------------------------------------------------------------ */
/* spread(flow) = the number of DISTINCT element keys inserted together with that
 * flow key since create / the last reset: len(spreadMap[key]) of the reference's
 * SuperSpread test (ss_test.go:49-66,86-136).  Exact: pairs are compared by their
 * bytes (never by a hash), a pair is counted once however its duplicates are
 * spread over lanes, workgroups, device batches and calls, and the result does
 * not depend on packet order.
 *   - Keys: flow and element keys are the EncodeFlow bytes SuperSpread uses for
 *     the same layout: task.go:265-300, IPv4 = 4 bytes + 12 zero bytes.  So a
 *     flow key taken from this engine is byte-for-byte a key gns_ss_query accepts
 *     and a Flow gns_ss_heavy_hitters returns.  This is deliberately NOT the exact
 *     aggregator's To16 form (gns_ex_*: ::ffff:a.b.c.d).
 *   - Records: gns_exs_insert_headers keeps, drops or counts a record as
 *     unsupported by the rules of gns_ss_insert_headers (the same parser); for the
 *     same input counters [0..2] equal SuperSpread's.
 *   - No traffic-dependent failure: the flow table and the pair table grow before
 *     a device batch that could fill them (max_flows / max_pairs are only the
 *     initial capacities); GNS_E_OOM only when the device cannot hold them (pair
 *     table limit 2^31 slots, flow table 2^30).
 *   - GNS_E_ARG at create: flow_bytes == 0, elem_bytes == 0, either above 37, more
 *     than 8 fields in a layout (checked before any device call).  With empty
 *     layouts (flow_bytes / elem_bytes alone) only gns_exs_insert_keys is usable.
 *   - Deviation from SuperSpread.Query (super_spread.go:238-258, minimum 1): a
 *     flow never seen answers 0. */
typedef struct gns_exs gns_exs;
typedef struct gns_exs_params {
    gns_layout flow, elem;   /* FlowFields / ElementFields */
    uint32_t flow_bytes, elem_bytes;
    uint64_t max_flows;      /* initial flow-table capacity (grows); 0 -> 1M */
    uint64_t max_pairs;      /* initial pair-table capacity (grows); 0 -> 4M */
    uint64_t batch_packets;  /* device batch; longer inserts are split; 0 -> 4M */
    int device;
} gns_exs_params;
int gns_exs_create(const gns_exs_params *p, gns_exs **out);
int gns_exs_destroy(gns_exs *h);
int gns_exs_insert_keys(gns_exs *h, const uint8_t *flows, uint32_t fstride, const uint8_t *elems,
                        uint32_t estride, uint64_t n, gns_mem where);
int gns_exs_insert_tuples(gns_exs *h, const gns_tuples *t, uint64_t n, gns_mem where);
int gns_exs_insert_headers(gns_exs *h, const uint8_t *hdr, const uint32_t *wirelen, uint64_t n,
                           gns_mem where);
/* Compact records, by the contract of gns_cm_insert_compact (see
 * gns_ss_insert_compact): equals gns_exs_insert_headers of the 64-byte records
 * the compact form was made from.  (Named outside the gns_exs_ family, whose symbol
 * list is pinned, as the gns_pairs_ calls are.) */
int gns_spread_insert_compact(gns_exs *h, const uint8_t *rec16, const uint32_t *wirelen, uint64_t n,
                           const uint8_t *side64, uint64_t n_side, gns_mem where);
int gns_exs_flush(gns_exs *h);
/* out[i] = spread of flow i (0 if never seen) */
int gns_exs_query(gns_exs *h, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
/* device keys / answers, as gns_ss_query_device */
int gns_exs_query_device(gns_exs *h, const uint8_t *flows, uint32_t stride, uint64_t n, uint64_t *out);
/* The flows with spread >= threshold, spread descending, ties by flow bytes
 * ascending (the shared list code of gns_cm_heavy_hitters).  *n = capacity in
 * (rows), full list length out; a list longer than its buffers is reported and
 * not written.  A threshold of 0 lists every seen flow (as 1 does). */
int gns_exs_heavy_hitters(gns_exs *h, uint32_t threshold, uint8_t *flows, uint32_t *spreads, uint64_t *n);
/* Every seen flow and its spread, in unspecified order; *n as above; NULL
 * buffers ask for the count only. */
int gns_exs_snapshot(gns_exs *h, uint8_t *flows, uint32_t *spreads, uint64_t *n);
/* empties both tables (they keep the size they have grown to); counters [0..4], [6], [7] keep counting */
int gns_exs_reset(gns_exs *h);
/* out[8]: inserted, dropped, unsupported, 0 (a probe without a free slot: cannot
 * happen), new pairs, flows now, records, device batches */
int gns_exs_counters(gns_exs *h, uint64_t out[8]);
/* [0] flow-table growths, [1] pair-table growths, [2] flow slots, [3] flow slots
 * claimed, [4] pair slots, [5] pair slots claimed, [6] growth time (us, host clock
 * incl. the device work), [7] 0 */
int gns_exs_dict_stats(gns_exs *h, uint64_t out[8]);
int gns_exs_set_timing(gns_exs *h, int on);
/* stages: 0 insert (first pass), 1 resolve rounds, 2 table growth, 3 roll-up projection
 * (the device work of gns_spread_rollup before its merge batches), 5 total (of a batch) */
int gns_exs_stage_times(gns_exs *h, double ms[8], uint64_t launches[8], int reset);

/* Pair set export and union: the exact spread engine's state interface.  A spread
 * count can neither be restored (later inserts need the pairs to tell a duplicate
 * from a new element) nor combined (the overlap is unknown); the set of distinct
 * (flow, element) pairs can: the union of two pair sets is exactly the pair set of
 * the concatenated streams, in any order and however the stream was split.
 *   - Export is a point in the stream: it runs on the handle's stream after
 *     everything issued so far; the exported rows grouped by flow are what the
 *     snapshot call of the handle returns, and a full export has dict_stats [5] rows.
 *   - Capacity: a count above *n on entry is reported with GNS_OK; rows at or past
 *     the capacity are not written (rows below it may be) and *cursor is not
 *     written.  Advance a cursor only on a written export and no pair is lost.
 *   - Delta: `since` is a cursor an earlier export or merge_from of the SAME handle
 *     returned; the result is exactly the pairs first inserted (or merged in) after
 *     that point.  Merged pairs count as inserted at the merge, so a collector that
 *     chains deltas passes them on.
 *   - Cursors are opaque and belong to a generation of the handle.  The reset call
 *     starts a new generation, and so does the wrap of the engine's 32-bit launch
 *     counter (every live record is then re-stamped as older than any new cursor).
 *     A cursor of another generation, or one the handle has not reached, is
 *     GNS_E_ARG: take a full export (since = 0).  GNS_EXS_TEST_EPOCH (environment,
 *     read at create, tests only) sets the starting launch counter.
 *   - Merge is a union, not traffic: counters [0], [1], [2], [6] and [7] do not move,
 *     [4] rises by the pairs actually added, [5] follows the flow table.  The tables
 *     grow before each piece as they do before a batch.
 *   - merge_from: dst == src, other key sizes or another device is GNS_E_ARG with
 *     dst untouched; src is read at a point of its own stream and not modified.
 *   - A null handle or a null n is GNS_E_ARG without a device. */
/* Every distinct (flow, element) pair the handle holds (since == 0), or only those first
 * inserted after the point `since` names: rows i of flows[*n * flow_bytes] and
 * elems[*n * elem_bytes], dense, unspecified order, host or device memory of the handle's GPU.
 * *n: capacity in rows on entry, the number of such pairs on return; NULL buffers ask for
 * the count only.  *cursor (may be NULL) names the point of the insert stream the export
 * was taken at: every insert and merge issued before the call is in, none after. */
int gns_pairs_export(gns_exs *h, uint64_t since, uint8_t *flows, uint8_t *elems, uint64_t *n,
                     uint64_t *cursor, gns_mem where);
/* Union: afterwards the handle holds its pairs and these.  Rows as the keys insert takes
 * them (strides >= the key sizes); duplicates inside the call and pairs already held count once. */
int gns_pairs_merge(gns_exs *h, const uint8_t *flows, uint32_t fstride, const uint8_t *elems,
                    uint32_t estride, uint64_t n, gns_mem where);
/* The export of src since `since`, merged into dst without the pairs leaving the device and
 * without a dense copy of the whole set (staged in pieces of 2^20 table slots).  *cursor
 * (may be NULL): src's point, for the next delta. */
int gns_pairs_merge_from(gns_exs *dst, gns_exs *src, uint64_t since, uint64_t *cursor);

/* Spread roll-up: the pair set of an exact spread table derived from the resident
 * flow table of an exact aggregator, on the device, after the traffic has gone.  The
 * distinct (flow, element) pairs of a stream are the projection of its distinct flow
 * keys whenever the flow and element fields are fields of the aggregator's key:
 * "distinct DstIPs per SrcIP", "distinct DstPorts per (SrcIP, DstIP)", and -- with
 * src's whole key as the element layout -- "flows per source address" all follow from
 * a five-tuple table.  (Named outside the gns_exs_ and gns_pairs_ families, whose symbol
 * lists are pinned, as gns_spread_insert_compact is.)
 *   - What it does.  Every flow gns_ex_snapshot(src) would list at the call (after
 *     src's pending batches) is projected onto dst's flow layout and onto dst's
 *     element layout, the two key rows are converted to EncodeFlow form, and the
 *     pairs enter dst as a union under the rules of gns_pairs_merge: duplicates
 *     inside the call and pairs already held count once; counters [0], [1], [2], [6]
 *     and [7] do not move, [4] rises by the pairs actually added, [5] follows the flow
 *     table; the tables grow before each device batch as in ingest; merged pairs are
 *     stamped with the merge's epoch, so gns_pairs_export(dst, since = ...) deltas
 *     pass them on.
 *   - Layouts.  Every field of dst's flow layout and of its element layout must
 *     occur in src's key layout, in any order; a field repeated in dst is copied once
 *     per occurrence, each from src's first occurrence (as gns_ex_rollup).  A dst
 *     created without field lists (flow_bytes / elem_bytes only) is refused: nothing
 *     names the fields to project.
 *   - Key form.  The aggregator stores IPs in To16 form, this engine in EncodeFlow
 *     form.  An IP field whose 16 bytes are ten zero bytes, ff ff, then a b c d is
 *     written as a b c d + 12 zero bytes; every other value is copied as is; ports
 *     and protocol are copied.  Consequence: into an empty dst the result equals a
 *     spread handle of those layouts fed the same packets -- keys, spreads, pair set
 *     and heavy list.  Deviation: a packet that carries an IPv4-mapped address in a
 *     16-byte net.IP is ONE key with the IPv4 address here (the aggregator already
 *     merged them, see gns_ex_*); it would be a separate key in a spread handle fed
 *     directly.  Note also that 0.0.0.0 and :: are both 16 zero bytes in EncodeFlow
 *     form, here as in a directly fed handle.
 *   - since / cursor.  since == 0 projects every flow.  since == a cursor this call
 *     or gns_ex_view_refresh returned for src projects only the flows whose first
 *     stream position is >= since: the flows new after that point.  A pair is new
 *     after that point only if every flow that projects onto it is new, so the delta
 *     projection is a superset of the new pairs and the union removes the rest;
 *     chaining since = the previous cursor into the same dst therefore keeps dst equal
 *     to a full roll-up.  *cursor (may be NULL) is src's next stream position
 *     (records inserted + rows merged), the value gns_ex_view_refresh returns; since
 *     beyond it is GNS_E_ARG.  Positions never restart: after gns_ex_reset(src) an old
 *     cursor selects every flow of the new period.  dst is a union: it keeps the
 *     pairs of earlier periods until the caller resets it.
 *   - out (may be NULL): [0] source flows projected, [1] pairs new in dst.
 *   - Calling rules.  Synchronous, and an ingest-side call on BOTH handles: no other
 *     thread may insert into src or dst during it.  src is read only: table, counters
 *     and cursors are unchanged.  src is read at an event of its own stream, by work
 *     on dst's stream (as gns_pairs_merge_from).  The work runs in pieces of 2^20
 *     source slots, gathered until more than a piece's worth of rows is staged and
 *     then merged in device batches of dst (GNS_SPREAD_ROLLUP_PIECE in the
 *     environment, read at the call, sets a smaller piece: for tests only, so that
 *     small tables span many pieces and merges).
 *   - GNS_E_ARG before any device call, dst untouched: a null handle, a dst without
 *     field lists, a dst field that src's key lacks (gns_last_error names it), handles
 *     on different devices, since beyond src's position.  An empty src is GNS_OK and
 *     moves nothing.
 *   - An error after the first merged batch (out of memory, a table at its slot
 *     limit) leaves dst with the pairs merged so far; a union is idempotent, so
 *     repeating the call is safe. */
int gns_spread_rollup(gns_exs *dst, gns_ex *src, uint64_t since, uint64_t *cursor, uint64_t out[2]);
/* Prefix spread roll-up: gns_spread_rollup with the IP fields of the flow row masked by
 * flow_px and those of the element row by elem_px (gns_prefix and its mask: see
 * gns_ex_rollup_prefix).  Both masks apply to the To16 bytes src stores, before the
 * EncodeFlow rewrite.  The two sides are separate because the prime uses read one field
 * twice under different masks:
 *   "distinct source hosts per source /24":  flow = SrcIP under {24,..}, element = SrcIP whole;
 *   "distinct /24s contacted per host":      flow = SrcIP whole, element = DstIP under {..,24,..}.
 * The result equals a spread handle of those layouts fed src's packets with their addresses
 * masked that way.  Everything else -- union semantics, counters, since / cursor (a delta is
 * a superset of the pairs that changed), out, pieces (GNS_SPREAD_ROLLUP_PIECE), the
 * IPv4-mapped deviation and the 0.0.0.0 / :: note -- is gns_spread_rollup's.  A prefix for a
 * field the row's layout lacks is ignored.  GNS_E_ARG, dst untouched: gns_spread_rollup's
 * cases; a null prefix, *_v4 > 32 or *_v6 > 128 (after the null-handle check and before
 * any device call). */
int gns_spread_rollup_prefix(gns_exs *dst, gns_ex *src, const gns_prefix *flow_px, const gns_prefix *elem_px,
                             uint64_t since, uint64_t *cursor, uint64_t out[2]);

/* Device buffers for callers without a device allocator of their own (the cgo
 * binding's ThriftDecoder: gns_thrift_decode writes device records that
 * gns_*_insert_headers then reads with GNS_MEM_DEVICE). */
int gns_device_alloc(uint64_t bytes, int device, void **out);
int gns_device_free(void *p, int device);

/* ---- self-test hooks ---- */
/* The device float64 helpers SuperSpread's sequential step inlines (csrc/gns_gomath.cuh),
 * evaluated over host arrays and returned to host arrays, so their roundings can be compared
 * with another restatement bit for bit.  Integers travel as the bit patterns of the doubles:
 *   GNS_GM_POW        out = go_pow_int(x, y)               Go math.Pow, integer y
 *   GNS_GM_LDEXP      out = go_ldexp(x, (int)(int64)bits(y))
 *   GNS_GM_FREXP      out, out2 = go_frexp(x)              out2 [n] int32, required
 *   GNS_GM_LOG        out = gm_log(x)                      x in (0, 1]
 *   GNS_GM_LOG1M      out = gm_log1m(x)                    0 < x < 1
 *   GNS_GM_UNIFORM    out = ss_uniform(seed, pkt = bits(x), row = bits(y) >> 32, draw = (u32)bits(y))
 *   GNS_GM_HLL_SEEDS  bits(out) = s1 << 32 | s0 of ss_hll_seeds(master = seed, cell = bits(x))
 * y is read by POW, LDEXP and UNIFORM only, out2 by FREXP only (NULL otherwise).
 * GNS_E_ARG: an unknown op, a null array the op needs, n > 2^30. */
enum { GNS_GM_POW = 0, GNS_GM_LDEXP, GNS_GM_FREXP, GNS_GM_LOG, GNS_GM_LOG1M, GNS_GM_UNIFORM, GNS_GM_HLL_SEEDS };
int gns_gomath_eval(int op, const double *x, const double *y, uint64_t n, double *out, int32_t *out2,
                    uint64_t seed, int device);

const char *gns_last_error(void);
const char *gns_version(void);

#ifdef __cplusplus
}
#endif
#endif
