// Package sketchgpu binds Go2NetSpectra's sketch aggregator to the MI355X engine
// (libgns_sketch.so, C ABI in include/gns_sketch.h) through cgo.
//
// It provides:
//   - CountMin: a statistic.Sketch (internal/engine/impl/sketch/statistic/sketch.go:5-10)
//     whose Insert/Query/HeavyHitters/Reset run on the GPU, plus InsertBatch for the
//     batched path;
//   - SuperSpread and Exact, the same way;
//   - task.go: GPUTask, a model.Task (internal/model/task.go:6-15) registered as the
//     "sketch_gpu" aggregator with factory.RegisterAggregator
//     (internal/factory/task_factory.go:24), whose ProcessPacket batches PacketInfo and
//     submits the batch with gns_{cm,ss}_insert_tuples instead of one CAS insert per
//     packet per worker.
//
// Build: CGO_CFLAGS="-I<repo>/include" CGO_LDFLAGS="-L<repo>/go2netspectra_amd -lgns_sketch".
// Not compiled in the build container (no Go toolchain there).
package sketchgpu

/*
#cgo LDFLAGS: -lgns_sketch
#include <stdlib.h>
#include "gns_sketch.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"log"
	"net"
	"sync"
	"unsafe"

	"Go2NetSpectra/internal/engine/impl/sketch/statistic"
)

var fieldIDs = map[string]C.uint8_t{"SrcIP": 1, "DstIP": 2, "SrcPort": 3, "DstPort": 4, "Protocol": 5}

func lastErr(rc C.int) error {
	if rc == C.GNS_OK {
		return nil
	}
	return errors.New(C.GoString(C.gns_last_error()))
}

// CountMin mirrors statistic.CountMin (count_min.go) on one GPU.
type CountMin struct {
	h        *C.gns_cm
	keyBytes int
	err      error // first insert failure of the period (Insert has no error return)
}

// sticky keeps the first failure of a measurement period and logs it the way
// the reference logs a dropped packet (task.go:162-166).  The engine has no
// traffic-dependent failure left (its flow dictionary grows, include/gns_sketch.h),
// so this reports device / runtime errors.
func sticky(dst *error, err error) {
	if err != nil && *dst == nil {
		*dst = err
		log.Printf("sketchgpu: insert failed, packets are dropped until Reset: %v", err)
	}
}

// NewCountMin replaces statistic.NewCountMin (count_min.go:47-90); seeds are injected.
func NewCountMin(width, depth, st, ct uint32, flowFields []string, keyBytes uint32, seeds []uint32,
	maxFlows uint64, device int) (*CountMin, error) {
	var p C.gns_cm_params
	p.width, p.depth = C.uint32_t(width), C.uint32_t(depth)
	p.size_threshold, p.count_threshold = C.uint32_t(st), C.uint32_t(ct)
	p.flow.n_fields = C.uint32_t(len(flowFields))
	for i, f := range flowFields {
		p.flow.fields[i] = fieldIDs[f]
	}
	p.key_bytes = C.uint32_t(keyBytes)
	if len(seeds) > 0 {
		p.seeds = (*C.uint32_t)(unsafe.Pointer(&seeds[0]))
	}
	p.max_flows = C.uint64_t(maxFlows)
	p.device = C.int(device)
	var h *C.gns_cm
	if err := lastErr(C.gns_cm_create(&p, &h)); err != nil {
		return nil, err
	}
	return &CountMin{h: h, keyBytes: int(keyBytes)}, nil
}

// Insert implements statistic.Sketch for one packet (a batch of one; prefer InsertBatch).
func (c *CountMin) Insert(flow, elem []byte, size uint32) {
	if len(flow) == 0 {
		return
	}
	sticky(&c.err, c.InsertBatch(flow, uint32(len(flow)), []uint32{size}))
}

// Err reports the first insert failure since the last Reset (nil if none).
func (c *CountMin) Err() error { return c.err }

// InsertBatch: keys is n*stride bytes, sizes n entries, applied in order.
func (c *CountMin) InsertBatch(keys []byte, stride uint32, sizes []uint32) error {
	if len(sizes) == 0 {
		return nil
	}
	return lastErr(C.gns_cm_insert_keys(c.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), C.uint32_t(stride),
		(*C.uint32_t)(unsafe.Pointer(&sizes[0])), C.uint64_t(len(sizes)), C.GNS_MEM_HOST))
}

// InsertTuples: PacketInfo batch as SoA (task.go:156-169 for a whole batch).
func (c *CountMin) InsertTuples(src16, dst16 []byte, sport, dport []uint16, proto []uint8, length []uint32) error {
	n := len(length)
	if n == 0 {
		return nil
	}
	t := C.gns_tuples{
		src16: (*C.uint8_t)(unsafe.Pointer(&src16[0])), dst16: (*C.uint8_t)(unsafe.Pointer(&dst16[0])),
		sport: (*C.uint16_t)(unsafe.Pointer(&sport[0])), dport: (*C.uint16_t)(unsafe.Pointer(&dport[0])),
		proto: (*C.uint8_t)(unsafe.Pointer(&proto[0])), length: (*C.uint32_t)(unsafe.Pointer(&length[0])),
	}
	return lastErr(C.gns_cm_insert_tuples(c.h, &t, C.uint64_t(n), C.GNS_MEM_HOST))
}

// InsertHeaders: 64-byte header records + wire lengths (PackCapture's output),
// parsed on the GPU (pcap.Reader.ReadPackets + ParsePacketInto + ProcessPacket).
func (c *CountMin) InsertHeaders(hdr []byte, wirelen []uint32) error {
	if len(wirelen) == 0 {
		return nil
	}
	return lastErr(C.gns_cm_insert_headers(c.h, (*C.uint8_t)(unsafe.Pointer(&hdr[0])),
		(*C.uint32_t)(unsafe.Pointer(&wirelen[0])), C.uint64_t(len(wirelen)), C.GNS_MEM_HOST))
}

// PackCapture replaces pcap.NewReader + Reader.ReadPackets (pkg/pcap/reader.go:20-49)
// on the ingest side: one pass over a classic pcap or pcapng file (what libpcap's
// pcap_open_offline reads) into 64-byte header records, wire lengths and capture
// timestamps in ns, ready for InsertHeaders.
func PackCapture(path string) (hdr []byte, wirelen []uint32, tsNs []int64, err error) {
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	var total C.uint64_t
	if r := C.gns_pack_pcap(cpath, nil, nil, 0, &total); r < 0 {
		return nil, nil, nil, lastErr(C.int(r))
	}
	n := int(total)
	if n == 0 {
		return nil, nil, nil, nil
	}
	hdr, wirelen, tsNs = make([]byte, 64*n), make([]uint32, n), make([]int64, n)
	r := C.gns_pack_pcap_ts(cpath, (*C.uint8_t)(unsafe.Pointer(&hdr[0])), (*C.uint32_t)(unsafe.Pointer(&wirelen[0])),
		(*C.int64_t)(unsafe.Pointer(&tsNs[0])), C.uint64_t(n), &total)
	if r < 0 {
		return nil, nil, nil, lastErr(C.int(r))
	}
	return hdr[:64*int(r)], wirelen[:r], tsNs[:r], nil
}

// FrameRecord is the live-capture form of PackCapture (pcap.OpenLive feeding
// gopacket.NewPacketSource): one captured frame (packet.Data(), CaptureInfo.Length
// as wireLen) -> the 64-byte record PackCapture writes for it. kind: 0 copied
// verbatim, 1 decoded on the host into a pre-parsed record, 2 no IP layer (the
// engine drops the record, as ParsePacketInto returns "not an IP packet").
func FrameRecord(frame []byte, wireLen uint32, rec []byte) (kind int, err error) {
	if len(rec) < 64 {
		return 0, errors.New("record buffer shorter than 64 bytes")
	}
	var p *C.uint8_t
	if len(frame) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&frame[0]))
	} else {
		p = (*C.uint8_t)(unsafe.Pointer(&rec[0])) // any non-nil pointer; caplen 0
	}
	r := C.gns_frame_record(p, C.uint32_t(len(frame)), C.uint32_t(wireLen), (*C.uint8_t)(unsafe.Pointer(&rec[0])))
	if r < 0 {
		return 0, lastErr(r)
	}
	return int(r), nil
}

// Reclaim drops flow-dictionary entries no bucket names any more (inserts also
// do it on their own when the dictionary fills); call it at a window boundary
// to take the rebuild off the ingest path.
func (c *CountMin) Reclaim() error { return lastErr(C.gns_cm_reclaim(c.h)) }

// DictStats: reclaims, dead flows dropped, live flows after the last reclaim,
// claimed slots, reclaim time (us), batches re-run after an overflow, slots, growths.
func (c *CountMin) DictStats() (out [8]uint64, err error) {
	err = lastErr(C.gns_cm_dict_stats(c.h, (*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return
}

func layoutOf(fields []string) (l C.gns_layout) {
	l.n_fields = C.uint32_t(len(fields))
	for i, f := range fields {
		l.fields[i] = fieldIDs[f]
	}
	return
}

// Router shards a node's traffic over its GPUs by flow (SURVEY §8e): records are
// split on the device by owning GPU (stable per shard; exchange the runs with an
// all-to-all and insert each received run in source-rank order), and queries are
// answered by the shard that owns the flow.  The owner key is the fields every
// task keys on (gns_route_owner_fields): [SrcIP] when each task's flow key holds
// SrcIP, otherwise the fields the tasks share -- for one task its whole flow key
// (a flow key without SrcIP is legal, config.go:59).
type Router struct {
	r       *C.gns_route
	nshards int
}

// NewRouter shards by SrcIP (every task keys on SrcIP).
func NewRouter(nshards uint32, device int) (*Router, error) {
	return NewKeyedRouter(nshards, [][]string{{"SrcIP"}}, device)
}

// NewKeyedRouter derives the owner key from the tasks' flow fields (one slice per
// task: SketchTaskDef.FlowFields / exact KeyFields); it fails when the tasks share
// no field, since no GPU could then own every flow of every task.
func NewKeyedRouter(nshards uint32, taskFields [][]string, device int) (*Router, error) {
	if len(taskFields) == 0 {
		return nil, errors.New("sketchgpu: no tasks to shard")
	}
	lays := make([]C.gns_layout, len(taskFields))
	for i, f := range taskFields {
		lays[i] = layoutOf(f)
	}
	var owner C.gns_layout
	if err := lastErr(C.gns_route_owner_fields(&lays[0], C.uint32_t(len(lays)), &owner)); err != nil {
		return nil, err
	}
	var r *C.gns_route
	if err := lastErr(C.gns_route_create_keyed(C.uint32_t(nshards), &owner, C.int(device), &r)); err != nil {
		return nil, err
	}
	return &Router{r: r, nshards: int(nshards)}, nil
}

// Partition: hdr/wirelen/outHdr/outWirelen are device pointers (n records);
// counts receives the run length of every shard.
func (rt *Router) Partition(hdr, wirelen, outHdr, outWirelen unsafe.Pointer, n uint64, counts []uint64) error {
	return lastErr(C.gns_route_partition(rt.r, (*C.uint8_t)(hdr), (*C.uint32_t)(wirelen), C.uint64_t(n),
		(*C.uint8_t)(outHdr), (*C.uint32_t)(outWirelen), (*C.uint64_t)(unsafe.Pointer(&counts[0]))))
}

// Owners returns the shard owning each of the len(keys)/stride flow keys (laid out as
// keyFields, the querying task's FlowFields; they must contain every owner field).
func (rt *Router) Owners(keyFields []string, keys []byte, stride uint32) ([]uint32, error) {
	if stride == 0 {
		return nil, errors.New("sketchgpu: zero key stride")
	}
	n := len(keys) / int(stride)
	own := make([]uint32, n+1)
	if n == 0 {
		return own[:0], nil
	}
	lay := layoutOf(keyFields)
	err := lastErr(C.gns_route_owner_keys(rt.r, &lay, (*C.uint8_t)(unsafe.Pointer(&keys[0])), C.uint32_t(stride),
		C.uint64_t(n), (*C.uint32_t)(unsafe.Pointer(&own[0])), C.GNS_MEM_HOST))
	return own[:n], err
}

// BatchQuerier is a shard's batched Query (CountMin, SuperSpread, Exact).
type BatchQuerier interface {
	QueryBatch(keys []byte, stride uint32) ([]uint64, error)
}

// QueryRouted answers Query(flow) (count_min.go:160-174, super_spread.go:238-249) for
// len(keys)/stride flow keys, each from the shard owning its flow: shards[g] is the
// handle on GPU g (one process driving the node's GPUs).  The shards answer
// concurrently, every key once; the answers come back in key order.
func (rt *Router) QueryRouted(shards []BatchQuerier, keyFields []string, keys []byte, stride uint32) ([]uint64, error) {
	if len(shards) != rt.nshards {
		return nil, fmt.Errorf("sketchgpu: %d shard handles for a %d-shard router", len(shards), rt.nshards)
	}
	own, err := rt.Owners(keyFields, keys, stride)
	if err != nil {
		return nil, err
	}
	per := make([][]int, rt.nshards)
	for i, g := range own {
		per[g] = append(per[g], i)
	}
	out := make([]uint64, len(own))
	errs := make([]error, rt.nshards)
	var wg sync.WaitGroup
	for g, idx := range per {
		if len(idx) == 0 {
			continue
		}
		wg.Add(1)
		go func(g int, idx []int) {
			defer wg.Done()
			buf := make([]byte, 0, len(idx)*int(stride))
			for _, i := range idx {
				buf = append(buf, keys[i*int(stride):(i+1)*int(stride)]...)
			}
			ans, err := shards[g].QueryBatch(buf, stride)
			if err != nil {
				errs[g] = err
				return
			}
			for j, i := range idx {
				out[i] = ans[j]
			}
		}(g, idx)
	}
	wg.Wait()
	for _, e := range errs {
		if e != nil {
			return nil, e
		}
	}
	return out, nil
}

func (rt *Router) Close() { C.gns_route_destroy(rt.r) }

// Query implements statistic.Sketch (count_min.go:160-174).
func (c *CountMin) Query(flow []byte) uint64 {
	if len(flow) != c.keyBytes || len(flow) == 0 {
		return 0
	}
	var out C.uint64_t
	if C.gns_cm_query(c.h, (*C.uint8_t)(unsafe.Pointer(&flow[0])), C.uint32_t(len(flow)), 1, &out) != C.GNS_OK {
		return 0
	}
	return uint64(out)
}

// QueryBatch: Query for len(keys)/stride flows in one device call (count<<32 | size).
func (c *CountMin) QueryBatch(keys []byte, stride uint32) ([]uint64, error) {
	n := len(keys) / int(stride)
	out := make([]uint64, n+1)
	if n == 0 {
		return out[:0], nil
	}
	err := lastErr(C.gns_cm_query(c.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), C.uint32_t(stride), C.uint64_t(n),
		(*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return out[:n], err
}

// HeavyHitters implements statistic.Sketch (count_min.go:178-247).
func (c *CountMin) HeavyHitters() statistic.HeavyRecord {
	return cmHeavy(c.keyBytes, func(cf *C.uint8_t, cv *C.uint32_t, nc *C.uint64_t, sf *C.uint8_t, sv *C.uint32_t,
		ns *C.uint64_t) C.int {
		return C.gns_cm_heavy_hitters(c.h, cf, cv, nc, sf, sv, ns)
	})
}

// cmHeavy runs a gns_cm_heavy_hitters-shaped call into Go buffers.  The call
// reports the full list lengths, which may exceed the buffers when the state
// changed since the sizing call (a View refreshed by its owner in between): the
// loop grows the buffers and calls again, so a list is never sliced past them.
func cmHeavy(K int, call func(cf *C.uint8_t, cv *C.uint32_t, nc *C.uint64_t, sf *C.uint8_t, sv *C.uint32_t,
	ns *C.uint64_t) C.int) statistic.HeavyRecord {
	empty := statistic.HeavyRecord{Size: []statistic.HeavySize{}, Count: []statistic.HeavyCount{}}
	capC, capS := 64, 64
	for tries := 0; tries < 8; tries++ {
		cf := make([]byte, capC*K+1)
		cv := make([]uint32, capC+1)
		sf := make([]byte, capS*K+1)
		sv := make([]uint32, capS+1)
		nc, ns := C.uint64_t(capC), C.uint64_t(capS)
		if call((*C.uint8_t)(unsafe.Pointer(&cf[0])), (*C.uint32_t)(unsafe.Pointer(&cv[0])), &nc,
			(*C.uint8_t)(unsafe.Pointer(&sf[0])), (*C.uint32_t)(unsafe.Pointer(&sv[0])), &ns) != C.GNS_OK {
			return empty
		}
		if int(nc) > capC || int(ns) > capS { // the lists outgrew the buffers: call again
			if int(nc) > capC {
				capC = 2 * int(nc)
			}
			if int(ns) > capS {
				capS = 2 * int(ns)
			}
			continue
		}
		rec := statistic.HeavyRecord{Size: make([]statistic.HeavySize, 0, int(ns)),
			Count: make([]statistic.HeavyCount, 0, int(nc))}
		for i := 0; i < int(ns); i++ {
			rec.Size = append(rec.Size, statistic.HeavySize{Flow: append([]byte(nil), sf[i*K:(i+1)*K]...), Size: sv[i]})
		}
		for i := 0; i < int(nc); i++ {
			rec.Count = append(rec.Count, statistic.HeavyCount{Flow: append([]byte(nil), cf[i*K:(i+1)*K]...), Count: cv[i]})
		}
		return rec
	}
	return empty
}

// Reset implements statistic.Sketch (count_min.go:249-265).
func (c *CountMin) Reset() {
	C.gns_cm_reset(c.h)
	c.err = nil
}

// Close releases the device sketch.
// ImportState replaces the sketch's whole state by arrays laid out as gns_cm_export_state
// writes them (C, S: depth*width counters; FPc, FPs: depth*width*keyBytes fingerprint
// bytes) -- a checkpoint taken from a sketch of the same geometry, key layout and seeds.
// counters: nil, or the new (inserted, dropped, unsupported).  Views taken before the call
// are stale until refreshed, as after Reset (gns_cm_import_state).
func (c *CountMin) ImportState(cnt, size []uint32, fpc, fps []byte, counters *[3]uint64) error {
	n := len(cnt)
	if n == 0 || len(size) != n || len(fpc) != n*c.keyBytes || len(fps) != n*c.keyBytes || c.keyBytes == 0 {
		return errors.New("sketchgpu: ImportState arrays do not match each other")
	}
	var cp *C.uint64_t
	if counters != nil {
		cp = (*C.uint64_t)(unsafe.Pointer(&counters[0]))
	}
	err := lastErr(C.gns_cm_import_state(c.h, (*C.uint32_t)(unsafe.Pointer(&cnt[0])),
		(*C.uint32_t)(unsafe.Pointer(&size[0])), (*C.uint8_t)(unsafe.Pointer(&fpc[0])),
		(*C.uint8_t)(unsafe.Pointer(&fps[0])), cp))
	if err == nil {
		c.err = nil
	}
	return err
}

func (c *CountMin) Close() { C.gns_cm_destroy(c.h) }

var _ statistic.Sketch = (*CountMin)(nil)

// View is a snapshot of a CountMin for the snapshotter / alerter goroutines
// (manager.go:139-159 call Snapshot while the workers insert): the worker that
// owns the CountMin calls Refresh at a window boundary, and any other goroutine
// may call HeavyHitters / Query on the view meanwhile (gns_cm_view_*).
type View struct {
	v        *C.gns_cm_view
	keyBytes int
}

// NewView allocates the snapshot (16 bytes per bucket).
func (c *CountMin) NewView() (*View, error) {
	var v *C.gns_cm_view
	if err := lastErr(C.gns_cm_view_create(c.h, &v)); err != nil {
		return nil, err
	}
	return &View{v: v, keyBytes: c.keyBytes}, nil
}

// Refresh snapshots the buckets after every insert issued so far (owner goroutine only).
func (w *View) Refresh() error { return lastErr(C.gns_cm_view_refresh(w.v)) }

// HeavyHitters is CountMin.HeavyHitters at the last Refresh, safe during inserts.
func (w *View) HeavyHitters() statistic.HeavyRecord {
	return cmHeavy(w.keyBytes, func(cf *C.uint8_t, cv *C.uint32_t, nc *C.uint64_t, sf *C.uint8_t, sv *C.uint32_t,
		ns *C.uint64_t) C.int {
		return C.gns_cm_view_heavy_hitters(w.v, cf, cv, nc, sf, sv, ns)
	})
}

// Query is CountMin.Query at the last Refresh, safe during inserts.
func (w *View) Query(flow []byte) uint64 {
	if len(flow) != w.keyBytes || len(flow) == 0 {
		return 0
	}
	var out C.uint64_t
	if C.gns_cm_view_query(w.v, (*C.uint8_t)(unsafe.Pointer(&flow[0])), C.uint32_t(len(flow)), 1, &out) != C.GNS_OK {
		return 0
	}
	return uint64(out)
}

// RefreshDetached snapshots like Refresh, and resolves the flows the buckets name into the
// view's own key table (gns_cm_view_refresh_at, GNS_CM_VIEW_DETACH): the snapshot then stays
// readable after the sketch's Reset, ImportState and dictionary reclaim until the next
// refresh -- the resetter is independent of the snapshotter (manager.go:161-193) -- and
// carries the counters for ExportState.  Owner goroutine only.
func (w *View) RefreshDetached() error {
	return lastErr(C.gns_cm_view_refresh_at(w.v, C.GNS_CM_VIEW_DETACH))
}

// QueryDevice answers n device-resident keys into device memory (gns_cm_view_query_device).
func (w *View) QueryDevice(keys unsafe.Pointer, stride uint32, n uint64, out unsafe.Pointer) error {
	return lastErr(C.gns_cm_view_query_device(w.v, (*C.uint8_t)(keys), C.uint32_t(stride), C.uint64_t(n),
		(*C.uint64_t)(out)))
}

// HeavyRows writes the two lists as packed device rows [flow | u32] (capacities capCount,
// capSize); it returns the full lengths, and writes no list that exceeds its capacity.
func (w *View) HeavyRows(countRows unsafe.Pointer, capCount uint64, sizeRows unsafe.Pointer,
	capSize uint64) (uint64, uint64, error) {
	nc, ns := C.uint64_t(capCount), C.uint64_t(capSize)
	err := lastErr(C.gns_cm_view_heavy_rows(w.v, (*C.uint8_t)(countRows), &nc, (*C.uint8_t)(sizeRows), &ns))
	return uint64(nc), uint64(ns), err
}

// ExportState returns the arrays CountMin.ImportState takes, as of the last refresh; cells =
// depth*width as given to NewCountMin (defaults resolved).  The counters need the last
// refresh to be RefreshDetached; withCounters false leaves them zero and works on either kind.
func (w *View) ExportState(cells int, withCounters bool) (cnt, size []uint32, fpc, fps []byte,
	counters [3]uint64, err error) {
	cnt = make([]uint32, cells+1)
	size = make([]uint32, cells+1)
	fpc = make([]byte, cells*w.keyBytes+1)
	fps = make([]byte, cells*w.keyBytes+1)
	var cp *C.uint64_t
	if withCounters {
		cp = (*C.uint64_t)(unsafe.Pointer(&counters[0]))
	}
	err = lastErr(C.gns_cm_view_export_state(w.v, (*C.uint32_t)(unsafe.Pointer(&cnt[0])),
		(*C.uint32_t)(unsafe.Pointer(&size[0])), (*C.uint8_t)(unsafe.Pointer(&fpc[0])),
		(*C.uint8_t)(unsafe.Pointer(&fps[0])), cp))
	return cnt[:cells], size[:cells], fpc[:cells*w.keyBytes], fps[:cells*w.keyBytes], counters, err
}

// Close releases the snapshot (before the CountMin it views).
func (w *View) Close() { C.gns_cm_view_destroy(w.v) }

// SuperSpread mirrors statistic.SuperSpread (super_spread.go) on one GPU.
type SuperSpread struct {
	h        *C.gns_ss
	flowSize int
	err      error // first insert failure of the period
}

// NewSuperSpread replaces statistic.NewSuperSpread (super_spread.go:129-149). Seeds, the
// HLL master seed and the declared generator's seed are injected (DESIGN.md §2).
func NewSuperSpread(width, depth, threshold, m, size uint32, base, b float64, flowFields, elemFields []string,
	seeds []uint32, hllMaster, rngSeed, maxFlows uint64, device int) (*SuperSpread, error) {
	var p C.gns_ss_params
	p.width, p.depth, p.threshold, p.m, p.size = C.uint32_t(width), C.uint32_t(depth), C.uint32_t(threshold),
		C.uint32_t(m), C.uint32_t(size)
	p.base, p.b = C.double(base), C.double(b)
	p.flow.n_fields = C.uint32_t(len(flowFields))
	for i, f := range flowFields {
		p.flow.fields[i] = fieldIDs[f]
	}
	p.elem.n_fields = C.uint32_t(len(elemFields))
	for i, f := range elemFields {
		p.elem.fields[i] = fieldIDs[f]
	}
	if len(seeds) > 0 {
		p.seeds = (*C.uint32_t)(unsafe.Pointer(&seeds[0]))
	}
	p.hll_master, p.rng_seed, p.device = C.uint64_t(hllMaster), C.uint64_t(rngSeed), C.int(device)
	p.max_flows = C.uint64_t(maxFlows) // 0 -> 4M
	var h *C.gns_ss
	if err := lastErr(C.gns_ss_create(&p, &h)); err != nil {
		return nil, err
	}
	fs := 0
	for _, f := range flowFields {
		fs += map[string]int{"SrcIP": 16, "DstIP": 16, "SrcPort": 2, "DstPort": 2, "Protocol": 1}[f]
	}
	return &SuperSpread{h: h, flowSize: fs}, nil
}

// InsertTuples: PacketInfo batch (task.go:156-169 for a whole batch).
func (s *SuperSpread) InsertTuples(src16, dst16 []byte, sport, dport []uint16, proto []uint8, length []uint32) error {
	n := len(length)
	if n == 0 {
		return nil
	}
	t := C.gns_tuples{
		src16: (*C.uint8_t)(unsafe.Pointer(&src16[0])), dst16: (*C.uint8_t)(unsafe.Pointer(&dst16[0])),
		sport: (*C.uint16_t)(unsafe.Pointer(&sport[0])), dport: (*C.uint16_t)(unsafe.Pointer(&dport[0])),
		proto: (*C.uint8_t)(unsafe.Pointer(&proto[0])), length: (*C.uint32_t)(unsafe.Pointer(&length[0])),
	}
	return lastErr(C.gns_ss_insert_tuples(s.h, &t, C.uint64_t(n), C.GNS_MEM_HOST))
}

// Insert implements statistic.Sketch for one packet (prefer InsertTuples).
func (s *SuperSpread) Insert(flow, elem []byte, size uint32) {
	if len(flow) == 0 {
		return
	}
	var e *C.uint8_t
	if len(elem) > 0 {
		e = (*C.uint8_t)(unsafe.Pointer(&elem[0]))
	}
	sticky(&s.err, lastErr(C.gns_ss_insert_keys(s.h, (*C.uint8_t)(unsafe.Pointer(&flow[0])),
		C.uint32_t(len(flow)), e, C.uint32_t(len(elem)), 1, C.GNS_MEM_HOST)))
}

// Err reports the first insert failure since the last Reset (nil if none).
func (s *SuperSpread) Err() error { return s.err }

// Query implements statistic.Sketch (super_spread.go:238-249).
func (s *SuperSpread) Query(flow []byte) uint64 {
	if len(flow) != s.flowSize || len(flow) == 0 {
		return 1
	}
	var out C.uint64_t
	if C.gns_ss_query(s.h, (*C.uint8_t)(unsafe.Pointer(&flow[0])), C.uint32_t(len(flow)), 1, &out) != C.GNS_OK {
		return 1
	}
	return uint64(out)
}

// QueryBatch: Query for len(keys)/stride flows in one device call.
func (s *SuperSpread) QueryBatch(keys []byte, stride uint32) ([]uint64, error) {
	n := len(keys) / int(stride)
	out := make([]uint64, n+1)
	if n == 0 {
		return out[:0], nil
	}
	err := lastErr(C.gns_ss_query(s.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), C.uint32_t(stride), C.uint64_t(n),
		(*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return out[:n], err
}

// HeavyHitters implements statistic.Sketch (super_spread.go:254-294): Size is nil.
func (s *SuperSpread) HeavyHitters() statistic.HeavyRecord {
	K := s.flowSize
	capN := 64
	for tries := 0; tries < 8; tries++ {
		fl := make([]byte, capN*K+1)
		v := make([]uint32, capN+1)
		n := C.uint64_t(capN)
		if C.gns_ss_heavy_hitters(s.h, (*C.uint8_t)(unsafe.Pointer(&fl[0])), (*C.uint32_t)(unsafe.Pointer(&v[0])),
			&n) != C.GNS_OK {
			break
		}
		if int(n) > capN { // longer than the buffers: grow and call again
			capN = 2 * int(n)
			continue
		}
		rec := statistic.HeavyRecord{Count: make([]statistic.HeavyCount, 0, int(n))}
		for i := 0; i < int(n); i++ {
			rec.Count = append(rec.Count, statistic.HeavyCount{Flow: append([]byte(nil), fl[i*K:(i+1)*K]...), Count: v[i]})
		}
		return rec
	}
	return statistic.HeavyRecord{Count: []statistic.HeavyCount{}}
}

// Reset implements statistic.Sketch (super_spread.go:297-311).
func (s *SuperSpread) Reset() {
	C.gns_ss_reset(s.h)
	s.err = nil
}

// Close releases the device sketch.
// ImportState replaces the sketch's whole state by arrays laid out as gns_ss_export_state
// writes them (values, keys, regs, pbits) plus records, the declared generator's position
// (gns_ss_counters [6]) -- without it a restored sketch draws other uniforms.  counters: nil,
// or the new (inserted, dropped, unsupported).  A register above 2^size - 1 is rejected
// before anything is written (gns_ss_import_state).
func (s *SuperSpread) ImportState(values []uint32, keys, regs []byte, pbits []float64, records uint64,
	counters *[3]uint64) error {
	n := len(values)
	if n == 0 || len(pbits) != n || len(keys) != n*s.flowSize || len(regs) == 0 || len(regs)%n != 0 || s.flowSize == 0 {
		return errors.New("sketchgpu: ImportState arrays do not match each other")
	}
	var cp *C.uint64_t
	if counters != nil {
		cp = (*C.uint64_t)(unsafe.Pointer(&counters[0]))
	}
	err := lastErr(C.gns_ss_import_state(s.h, (*C.uint32_t)(unsafe.Pointer(&values[0])),
		(*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint8_t)(unsafe.Pointer(&regs[0])),
		(*C.double)(unsafe.Pointer(&pbits[0])), C.uint64_t(records), cp))
	if err == nil {
		s.err = nil
	}
	return err
}

func (s *SuperSpread) Close() { C.gns_ss_destroy(s.h) }

var _ statistic.Sketch = (*SuperSpread)(nil)

// SuperSpreadView is a snapshot view of a SuperSpread (gns_ss_view_*) for the snapshotter and
// alerter goroutines (manager.go:139-159): Refresh on the goroutine that inserts, at the
// interval's end; Query, HeavyHitters and ExportState on any other while the inserts go on.
// Every answer is the sketch's at the Refresh.  The view holds key bytes, so it stays readable
// after the sketch's Reset (the resetter is independent of the snapshotter).  Close views
// before their sketch.
type SuperSpreadView struct {
	v        *C.gns_ss_view
	flowSize int
	cells    int
	m        int
}

// NewView creates a view of s; cells = depth*width and m as given to NewSuperSpread (their
// defaults resolved) size ExportState's arrays.
func (s *SuperSpread) NewView(cells, m int) (*SuperSpreadView, error) {
	var v *C.gns_ss_view
	if err := lastErr(C.gns_ss_view_create(s.h, &v)); err != nil {
		return nil, err
	}
	return &SuperSpreadView{v: v, flowSize: s.flowSize, cells: cells, m: m}, nil
}

// Refresh snapshots the cells after every insert issued so far (asynchronous, insert side).
// state: also registers, pbits, counters and the generator position, for ExportState.
func (w *SuperSpreadView) Refresh(state bool) error {
	var flags C.uint32_t
	if state {
		flags = C.GNS_SS_VIEW_STATE
	}
	return lastErr(C.gns_ss_view_refresh(w.v, flags))
}

// Query is SuperSpread.Query at the Refresh.
func (w *SuperSpreadView) Query(flow []byte) uint64 {
	if len(flow) != w.flowSize || len(flow) == 0 {
		return 1
	}
	var out C.uint64_t
	if C.gns_ss_view_query(w.v, (*C.uint8_t)(unsafe.Pointer(&flow[0])), C.uint32_t(len(flow)), 1, &out) != C.GNS_OK {
		return 1
	}
	return uint64(out)
}

// QueryDevice answers n device-resident keys into device memory (gns_ss_view_query_device).
func (w *SuperSpreadView) QueryDevice(keys unsafe.Pointer, stride uint32, n uint64, out unsafe.Pointer) error {
	return lastErr(C.gns_ss_view_query_device(w.v, (*C.uint8_t)(keys), C.uint32_t(stride), C.uint64_t(n),
		(*C.uint64_t)(out)))
}

// HeavyHitters is SuperSpread.HeavyHitters at the Refresh: Size is nil.
func (w *SuperSpreadView) HeavyHitters() (statistic.HeavyRecord, error) {
	K := w.flowSize
	capN := 64
	for {
		fl := make([]byte, capN*K+1)
		v := make([]uint32, capN+1)
		n := C.uint64_t(capN)
		if err := lastErr(C.gns_ss_view_heavy_hitters(w.v, (*C.uint8_t)(unsafe.Pointer(&fl[0])),
			(*C.uint32_t)(unsafe.Pointer(&v[0])), &n)); err != nil {
			return statistic.HeavyRecord{Count: []statistic.HeavyCount{}}, err
		}
		if int(n) > capN { // longer than the buffers: grow and call again
			capN = 2 * int(n)
			continue
		}
		rec := statistic.HeavyRecord{Count: make([]statistic.HeavyCount, 0, int(n))}
		for i := 0; i < int(n); i++ {
			rec.Count = append(rec.Count, statistic.HeavyCount{Flow: append([]byte(nil), fl[i*K:(i+1)*K]...), Count: v[i]})
		}
		return rec, nil
	}
}

// HeavyRows writes the list as packed device rows [flow | u32] (capacity capRows); it
// returns the full length, and writes nothing when that exceeds the capacity.
func (w *SuperSpreadView) HeavyRows(rowsDev unsafe.Pointer, capRows uint64) (uint64, error) {
	n := C.uint64_t(capRows)
	err := lastErr(C.gns_ss_view_heavy_rows(w.v, (*C.uint8_t)(rowsDev), &n))
	return uint64(n), err
}

// ExportState returns the arrays SuperSpread.ImportState takes, as of the last Refresh(true).
func (w *SuperSpreadView) ExportState() (values []uint32, keys, regs []byte, pbits []float64, records uint64,
	counters [3]uint64, err error) {
	values = make([]uint32, w.cells+1)
	keys = make([]byte, w.cells*w.flowSize+1)
	regs = make([]byte, w.cells*w.m+1)
	pbits = make([]float64, w.cells+1)
	var rec C.uint64_t
	err = lastErr(C.gns_ss_view_export_state(w.v, (*C.uint32_t)(unsafe.Pointer(&values[0])),
		(*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint8_t)(unsafe.Pointer(&regs[0])),
		(*C.double)(unsafe.Pointer(&pbits[0])), &rec, (*C.uint64_t)(unsafe.Pointer(&counters[0]))))
	return values[:w.cells], keys[:w.cells*w.flowSize], regs[:w.cells*w.m], pbits[:w.cells], uint64(rec), counters, err
}

// Close releases the view.
func (w *SuperSpreadView) Close() { C.gns_ss_view_destroy(w.v) }

// Exact is the device state of one exact task (internal/engine/impl/exact/task.go).
type Exact struct {
	h        *C.gns_ex
	keyBytes int
}

// NewExact replaces exact.New's flow map (task.go:83-103).
func NewExact(keyFields []string, maxFlows uint64, device int) (*Exact, error) {
	var p C.gns_ex_params
	p.key.n_fields = C.uint32_t(len(keyFields))
	kb := 0
	for i, f := range keyFields {
		p.key.fields[i] = fieldIDs[f]
		kb += map[string]int{"SrcIP": 16, "DstIP": 16, "SrcPort": 2, "DstPort": 2, "Protocol": 1}[f]
	}
	p.max_flows, p.device = C.uint64_t(maxFlows), C.int(device)
	var h *C.gns_ex
	if err := lastErr(C.gns_ex_create(&p, &h)); err != nil {
		return nil, err
	}
	return &Exact{h: h, keyBytes: kb}, nil
}

// InsertTuples is ProcessPacket (task.go:124-149) for a batch; ipver[i] = len(IP) == 4 ? 4 : 6.
func (e *Exact) InsertTuples(src16, dst16 []byte, sport, dport []uint16, proto []uint8, length []uint32,
	ipver []uint8, tsNano []int64) error {
	n := len(length)
	if n == 0 {
		return nil
	}
	t := C.gns_tuples{
		src16: (*C.uint8_t)(unsafe.Pointer(&src16[0])), dst16: (*C.uint8_t)(unsafe.Pointer(&dst16[0])),
		sport: (*C.uint16_t)(unsafe.Pointer(&sport[0])), dport: (*C.uint16_t)(unsafe.Pointer(&dport[0])),
		proto: (*C.uint8_t)(unsafe.Pointer(&proto[0])), length: (*C.uint32_t)(unsafe.Pointer(&length[0])),
	}
	return lastErr(C.gns_ex_insert_tuples(e.h, &t, (*C.uint8_t)(unsafe.Pointer(&ipver[0])),
		(*C.int64_t)(unsafe.Pointer(&tsNano[0])), C.uint64_t(n), C.GNS_MEM_HOST))
}

// Query is exact.Task.Query (task.go:298-326).
func (e *Exact) Query(flow []byte) uint64 {
	if len(flow) != e.keyBytes || len(flow) == 0 {
		return 0
	}
	var out C.uint64_t
	if C.gns_ex_query(e.h, (*C.uint8_t)(unsafe.Pointer(&flow[0])), C.uint32_t(len(flow)), 1, &out) != C.GNS_OK {
		return 0
	}
	return uint64(out)
}

// QueryBatch: Query for len(keys)/stride flows in one device call (PacketCount<<32 | ByteCount).
func (e *Exact) QueryBatch(keys []byte, stride uint32) ([]uint64, error) {
	n := len(keys) / int(stride)
	out := make([]uint64, n+1)
	if n == 0 {
		return out[:0], nil
	}
	err := lastErr(C.gns_ex_query(e.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), C.uint32_t(stride), C.uint64_t(n),
		(*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return out[:n], err
}

// Flows returns the snapshot arrays; the task rebuilds statistic.Flow (Key string via
// net.IP(key[i:i+16]).String(), Fields, StartTime = time.Unix(0, start[i]), ...).
func (e *Exact) Flows() (keys []byte, start, end []int64, pkts, bytes []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_snapshot(e.h, nil, nil, nil, nil, nil, &n)); err != nil {
		return
	}
	m := int(n)
	keys = make([]byte, m*e.keyBytes+1)
	start, end = make([]int64, m+1), make([]int64, m+1)
	pkts, bytes = make([]uint64, m+1), make([]uint64, m+1)
	err = lastErr(C.gns_ex_snapshot(e.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.int64_t)(unsafe.Pointer(&start[0])),
		(*C.int64_t)(unsafe.Pointer(&end[0])), (*C.uint64_t)(unsafe.Pointer(&pkts[0])),
		(*C.uint64_t)(unsafe.Pointer(&bytes[0])), &n))
	m = int(n)
	return keys[:m*e.keyBytes], start[:m], end[:m], pkts[:m], bytes[:m], err
}

// ExactFilter is the equality filter of query.AggregationRequest and of
// TraceFlowRequest.FlowKeys (internal/query/querier.go:19-26, :143-188): a nil field is open,
// every other field must equal the flow's.  A field that is not part of the task's key
// matches no flow (the reference stores that column as NULL).
type ExactFilter struct {
	SrcIP, DstIP     net.IP
	SrcPort, DstPort *uint16
	Protocol         *uint8
}

// ExactSummary is gns_ex_summary: AggregateFlows' COUNT / SUM columns (querier.go:251-319)
// and TraceFlow's min / max columns (querier.go:322-372) of the flows one filter matches.
type ExactSummary struct {
	Flows, Packets, Bytes uint64
	FirstNs, LastNs       int64 // time.Unix(0, ns); 0, 0 when Flows == 0
	MaxPackets, MaxBytes  uint64
}

func exactFilterIP(dst *[16]C.uint8_t, ip net.IP) error {
	ip16 := ip.To16()
	if ip16 == nil {
		return fmt.Errorf("sketchgpu: IP of %d bytes in an exact filter", len(ip))
	}
	for i := 0; i < 16; i++ {
		dst[i] = C.uint8_t(ip16[i])
	}
	return nil
}

// exactFilters lays the filters out as gns_ex_filter.
func exactFilters(filters []ExactFilter) ([]C.gns_ex_filter, error) {
	cf := make([]C.gns_ex_filter, len(filters))
	for i, f := range filters {
		if f.SrcIP != nil {
			if err := exactFilterIP(&cf[i].src16, f.SrcIP); err != nil {
				return nil, err
			}
			cf[i].mask |= 1 << C.GNS_F_SRCIP
		}
		if f.DstIP != nil {
			if err := exactFilterIP(&cf[i].dst16, f.DstIP); err != nil {
				return nil, err
			}
			cf[i].mask |= 1 << C.GNS_F_DSTIP
		}
		if f.SrcPort != nil {
			cf[i].sport = C.uint16_t(*f.SrcPort)
			cf[i].mask |= 1 << C.GNS_F_SRCPORT
		}
		if f.DstPort != nil {
			cf[i].dport = C.uint16_t(*f.DstPort)
			cf[i].mask |= 1 << C.GNS_F_DSTPORT
		}
		if f.Protocol != nil {
			cf[i].proto = C.uint8_t(*f.Protocol)
			cf[i].mask |= 1 << C.GNS_F_PROTO
		}
	}
	return cf, nil
}

func exactSummaries(cs []C.gns_ex_summary) []ExactSummary {
	out := make([]ExactSummary, len(cs))
	for i, s := range cs {
		out[i] = ExactSummary{Flows: uint64(s.flows), Packets: uint64(s.packets), Bytes: uint64(s.bytes),
			FirstNs: int64(s.first_ns), LastNs: int64(s.last_ns),
			MaxPackets: uint64(s.max_packets), MaxBytes: uint64(s.max_bytes)}
	}
	return out
}

// Aggregate answers every filter from one device scan per 64 filters (gns_ex_aggregate):
// AggregateFlows and TraceFlow on the live table, without a snapshot leaving the GPU.
func (e *Exact) Aggregate(filters []ExactFilter) ([]ExactSummary, error) {
	n := len(filters)
	if n == 0 {
		return nil, nil
	}
	cf, err := exactFilters(filters)
	if err != nil {
		return nil, err
	}
	cs := make([]C.gns_ex_summary, n)
	if err := lastErr(C.gns_ex_aggregate(e.h, &cf[0], C.uint32_t(n), &cs[0])); err != nil {
		return nil, err
	}
	return exactSummaries(cs), nil
}

// HeavyHitters is QueryHeavyHitters (querier.go:191-248) on the live table (gns_ex_heavy_hitters):
// the flows with PacketCount (metric 0) or ByteCount (metric 1) >= threshold, value descending,
// ties by key bytes ascending, cut to limit rows when limit != 0.  keys holds len(values) keys
// of the task's key bytes each, in the layout of Flows.
func (e *Exact) HeavyHitters(metric int, threshold, limit uint64) (keys []byte, values []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_heavy_hitters(e.h, C.int(metric), C.uint64_t(threshold), C.uint64_t(limit),
		nil, nil, &n)); err != nil || n == 0 {
		return nil, nil, err
	}
	m := int(n)
	keys, values = make([]byte, m*e.keyBytes+1), make([]uint64, m)
	err = lastErr(C.gns_ex_heavy_hitters(e.h, C.int(metric), C.uint64_t(threshold), C.uint64_t(limit),
		(*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint64_t)(unsafe.Pointer(&values[0])), &n))
	if err == nil && int(n) != m {
		err = fmt.Errorf("sketchgpu: heavy-hitter list changed length between calls (%d, %d)", m, int(n))
	}
	return keys[:m*e.keyBytes], values, err
}

// Merge adds rows laid out as Flows returns them to the table (gns_ex_merge): each row is one
// pseudo-record at the current end of the stream, so a new key takes the row's start and end,
// an existing key keeps its start and takes the row's end, and the counts add.  Rows without
// packets are ignored.  A restore is a Merge into an empty table; the union of two shards is a
// Merge of one's Flows into the other.
func (e *Exact) Merge(keys []byte, start, end []int64, pkts, bytes []uint64) error {
	n := len(pkts)
	if n == 0 {
		return nil
	}
	if len(keys) != n*e.keyBytes || len(start) != n || len(end) != n || len(bytes) != n {
		return errors.New("sketchgpu: Merge arrays do not match each other")
	}
	return lastErr(C.gns_ex_merge(e.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.int64_t)(unsafe.Pointer(&start[0])),
		(*C.int64_t)(unsafe.Pointer(&end[0])), (*C.uint64_t)(unsafe.Pointer(&pkts[0])),
		(*C.uint64_t)(unsafe.Pointer(&bytes[0])), C.uint64_t(n), C.GNS_MEM_HOST))
}

// RollupFrom re-keys the flows of src onto this table's key layout on the device
// (gns_ex_rollup): the flows of src that share one projected key enter as one pseudo-record
// under the rule of Merge, with the group's summed counts, the start of its earliest and the
// end of its latest constituent in src's stream order.  Every field of this table's layout
// must be part of src's.  Into an empty table the result equals a task keyed on this layout
// and fed src's packets.  src is only read; neither table may take inserts during the call.
// projected = flows of src, added = flows new in this table.
func (e *Exact) RollupFrom(src *Exact) (projected, added uint64, err error) {
	if src == nil {
		return 0, 0, errors.New("sketchgpu: RollupFrom of a nil source")
	}
	var out [2]C.uint64_t
	if err = lastErr(C.gns_ex_rollup(e.h, src.h, &out[0])); err != nil {
		return 0, 0, err
	}
	return uint64(out[0]), uint64(out[1]), nil
}

// Prefix is gns_prefix: the leading bits kept of SrcIP and DstIP by a prefix roll-up, per
// address class.  A value that is IPv4 in its To16 form (::ffff:a.b.c.d) keeps its leading
// SrcV4 / DstV4 bits (0..32), every other value its leading SrcV6 / DstV6 bits (0..128).
// FullPrefix keeps everything.
type Prefix struct {
	SrcV4, SrcV6, DstV4, DstV6 uint8
}

// FullPrefix masks nothing: RollupPrefixFrom with it equals RollupFrom.
var FullPrefix = Prefix{32, 128, 32, 128}

// RollupPrefixFrom is RollupFrom with the projected key's IP fields masked to px
// (gns_ex_rollup_prefix): "bytes per source /24" is a table keyed on SrcIP rolled up with
// Prefix{24, 64, 32, 128}.  Into an empty table the result equals a task keyed on this layout
// and fed src's packets with their addresses masked.  A prefix for a field this layout lacks is
// ignored.  The result is a full table, and can itself be the source of a coarser roll-up.
func (e *Exact) RollupPrefixFrom(src *Exact, px Prefix) (projected, added uint64, err error) {
	if src == nil {
		return 0, 0, errors.New("sketchgpu: RollupPrefixFrom of a nil source")
	}
	cp := C.gns_prefix{src_v4: C.uint8_t(px.SrcV4), src_v6: C.uint8_t(px.SrcV6), dst_v4: C.uint8_t(px.DstV4),
		dst_v6: C.uint8_t(px.DstV6)}
	var out [2]C.uint64_t
	if err = lastErr(C.gns_ex_rollup_prefix(e.h, src.h, &cp, &out[0])); err != nil {
		return 0, 0, err
	}
	return uint64(out[0]), uint64(out[1]), nil
}

// ExactCIDR is gns_ex_cidr: an ExactFilter whose SrcIP / DstIP, when set, need not match in
// their trailing SrcHostBits / DstHostBits bits (0..128 of the 16-byte To16 form).  The zero
// value is ExactFilter's equality, so ExactCIDR{ExactFilter: f} selects what f selects; an IPv4
// /24 is 8 host bits, an IPv6 /48 is 80, and 128 matches every flow whose key has the field.
// Address bits inside the host part are ignored.
type ExactCIDR struct {
	ExactFilter
	SrcHostBits, DstHostBits uint8
}

// CIDROf is the ExactCIDR of a net.IPNet per address (nil: the field stays open).
func CIDROf(src, dst *net.IPNet) ExactCIDR {
	var c ExactCIDR
	if src != nil {
		ones, bits := src.Mask.Size()
		c.SrcIP, c.SrcHostBits = src.IP, uint8(bits-ones)
	}
	if dst != nil {
		ones, bits := dst.Mask.Size()
		c.DstIP, c.DstHostBits = dst.IP, uint8(bits-ones)
	}
	return c
}

// exactCIDRs lays the filters out as gns_ex_cidr.
func exactCIDRs(filters []ExactCIDR) ([]C.gns_ex_cidr, error) {
	plain := make([]ExactFilter, len(filters))
	for i, f := range filters {
		plain[i] = f.ExactFilter
	}
	cf, err := exactFilters(plain)
	if err != nil {
		return nil, err
	}
	cc := make([]C.gns_ex_cidr, len(filters))
	for i, f := range filters {
		if f.SrcHostBits > 128 || f.DstHostBits > 128 {
			return nil, fmt.Errorf("sketchgpu: filter %d: %d / %d host bits of a 128-bit address", i, f.SrcHostBits, f.DstHostBits)
		}
		cc[i].f = cf[i]
		cc[i].src_bits, cc[i].dst_bits = C.uint8_t(128-f.SrcHostBits), C.uint8_t(128-f.DstHostBits)
	}
	return cc, nil
}

// AggregateCIDR is Aggregate with prefix matches on the IP fields (gns_ex_aggregate_cidr).
func (e *Exact) AggregateCIDR(filters []ExactCIDR) ([]ExactSummary, error) {
	n := len(filters)
	if n == 0 {
		return nil, nil
	}
	cc, err := exactCIDRs(filters)
	if err != nil {
		return nil, err
	}
	cs := make([]C.gns_ex_summary, n)
	if err := lastErr(C.gns_ex_aggregate_cidr(e.h, &cc[0], C.uint32_t(n), &cs[0])); err != nil {
		return nil, err
	}
	return exactSummaries(cs), nil
}

// Reset is exact.Task.Reset (task.go:194-210).
func (e *Exact) Reset() { C.gns_ex_reset(e.h) }

// Close releases the device state.
func (e *Exact) Close() { C.gns_ex_destroy(e.h) }

// ExactView is a snapshot view of an Exact (gns_ex_view_*) for the snapshotter and alerter
// goroutines (manager.go:139-159, exact/task.go:154-194, :224-233): a dense copy of the
// table, or of the flows touched since a cursor, taken by Refresh on the ingest goroutine
// and read by Flows / Aggregate / HeavyHitters on any other goroutine while the task keeps
// inserting.  It stays what it was at the Refresh whatever the Exact does afterwards, Reset
// included.  Close it before its Exact.
type ExactView struct {
	v        *C.gns_ex_view
	keyBytes int
}

// NewView allocates an empty view; its tables are sized by the first Refresh.
func (e *Exact) NewView() (*ExactView, error) {
	var v *C.gns_ex_view
	if err := lastErr(C.gns_ex_view_create(e.h, &v)); err != nil {
		return nil, err
	}
	return &ExactView{v: v, keyBytes: e.keyBytes}, nil
}

// Refresh selects, as of every InsertTuples and Merge issued so far, the flows touched after
// the cursor since (0: every flow) and returns the cursor of this point for the next call.
// Rows are cumulative, and the store keeps the latest row per flow, so a writer may store
// only each interval's delta.  Ingest side: call it where the Exact's other calls are made.
func (w *ExactView) Refresh(since uint64) (cursor uint64, err error) {
	var c C.uint64_t
	err = lastErr(C.gns_ex_view_refresh(w.v, C.uint64_t(since), &c))
	return uint64(c), err
}

// Flows returns the view's rows in the layout of Exact.Flows (after Refresh(0): the arrays
// Exact.Flows returned at that point).
func (w *ExactView) Flows() (keys []byte, start, end []int64, pkts, bytes []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_view_snapshot(w.v, nil, nil, nil, nil, nil, &n)); err != nil {
		return
	}
	m := int(n)
	keys = make([]byte, m*w.keyBytes+1)
	start, end = make([]int64, m+1), make([]int64, m+1)
	pkts, bytes = make([]uint64, m+1), make([]uint64, m+1)
	err = lastErr(C.gns_ex_view_snapshot(w.v, (*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.int64_t)(unsafe.Pointer(&start[0])),
		(*C.int64_t)(unsafe.Pointer(&end[0])), (*C.uint64_t)(unsafe.Pointer(&pkts[0])),
		(*C.uint64_t)(unsafe.Pointer(&bytes[0])), &n))
	m = int(n)
	return keys[:m*w.keyBytes], start[:m], end[:m], pkts[:m], bytes[:m], err
}

// Aggregate is Exact.Aggregate over the view's rows (the alerter's totals: one open filter).
func (w *ExactView) Aggregate(filters []ExactFilter) ([]ExactSummary, error) {
	n := len(filters)
	if n == 0 {
		return nil, nil
	}
	cf, err := exactFilters(filters)
	if err != nil {
		return nil, err
	}
	cs := make([]C.gns_ex_summary, n)
	if err := lastErr(C.gns_ex_view_aggregate(w.v, &cf[0], C.uint32_t(n), &cs[0])); err != nil {
		return nil, err
	}
	return exactSummaries(cs), nil
}

// AggregateCIDR is Exact.AggregateCIDR over the view's rows (gns_ex_view_aggregate_cidr).
func (w *ExactView) AggregateCIDR(filters []ExactCIDR) ([]ExactSummary, error) {
	n := len(filters)
	if n == 0 {
		return nil, nil
	}
	cc, err := exactCIDRs(filters)
	if err != nil {
		return nil, err
	}
	cs := make([]C.gns_ex_summary, n)
	if err := lastErr(C.gns_ex_view_aggregate_cidr(w.v, &cc[0], C.uint32_t(n), &cs[0])); err != nil {
		return nil, err
	}
	return exactSummaries(cs), nil
}

// HeavyHitters is Exact.HeavyHitters over the view's rows.
func (w *ExactView) HeavyHitters(metric int, threshold, limit uint64) (keys []byte, values []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_view_heavy_hitters(w.v, C.int(metric), C.uint64_t(threshold), C.uint64_t(limit),
		nil, nil, &n)); err != nil || n == 0 {
		return nil, nil, err
	}
	m := int(n)
	keys, values = make([]byte, m*w.keyBytes+1), make([]uint64, m)
	err = lastErr(C.gns_ex_view_heavy_hitters(w.v, C.int(metric), C.uint64_t(threshold), C.uint64_t(limit),
		(*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint64_t)(unsafe.Pointer(&values[0])), &n))
	return keys[:m*w.keyBytes], values, err
}

// Close releases the view.
func (w *ExactView) Close() { C.gns_ex_view_destroy(w.v) }

// History is the store behind the Querier's EndTime (gns_ex_hist_*): an append-only log, on
// the device, of the rows the snapshotter hands to the writer each interval
// (manager.go:139-159).  Append stores one refreshed ExactView -- whole or delta -- under a
// Timestamp; every query takes an end time and answers as of the newest snapshot at or
// before it (`Timestamp <= ?`, querier.go:211-213, 271-273, 344-346): per flow its latest row
// by then, argMax(..., Timestamp).  A nil end time is the newest snapshot.  Calls may come
// from any goroutine.
type History struct {
	h        *C.gns_ex_hist
	keyBytes int
}

// NewHistory allocates a history for views of an Exact with the same key fields.  maxRows and
// maxFlows are initial capacities (0: defaults); both grow.
func NewHistory(keyFields []string, maxRows, maxFlows uint64, device int) (*History, error) {
	var p C.gns_ex_hist_params
	p.key.n_fields = C.uint32_t(len(keyFields))
	kb := 0
	for i, f := range keyFields {
		p.key.fields[i] = fieldIDs[f]
		kb += map[string]int{"SrcIP": 16, "DstIP": 16, "SrcPort": 2, "DstPort": 2, "Protocol": 1}[f]
	}
	p.max_rows, p.max_flows, p.device = C.uint64_t(maxRows), C.uint64_t(maxFlows), C.int(device)
	var h *C.gns_ex_hist
	if err := lastErr(C.gns_ex_hist_create(&p, &h)); err != nil {
		return nil, err
	}
	return &History{h: h, keyBytes: kb}, nil
}

func endNs(end *int64) *C.int64_t { return (*C.int64_t)(unsafe.Pointer(end)) }

// Append stores the view's rows as the next snapshot; tsNano must lie after the last one's.
// A reader call on the view: it may run on the snapshotter goroutine while the Exact ingests.
func (y *History) Append(w *ExactView, tsNano int64) (rows, newKeys uint64, err error) {
	var out [2]C.uint64_t
	err = lastErr(C.gns_ex_hist_append(y.h, w.v, C.int64_t(tsNano), &out[0]))
	return uint64(out[0]), uint64(out[1]), err
}

// Times returns the snapshots' timestamps.
func (y *History) Times() ([]int64, error) {
	var n C.uint64_t
	if err := lastErr(C.gns_ex_hist_times(y.h, nil, &n)); err != nil || n == 0 {
		return nil, err
	}
	ts := make([]int64, int(n))
	err := lastErr(C.gns_ex_hist_times(y.h, (*C.int64_t)(unsafe.Pointer(&ts[0])), &n))
	if int(n) < len(ts) {
		ts = ts[:int(n)]
	}
	return ts, err
}

// Stats returns snapshots, rows, distinct keys, row capacity, index slots, index growths, log growths, 0.
func (y *History) Stats() (out [8]uint64, err error) {
	err = lastErr(C.gns_ex_hist_stats(y.h, (*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return
}

// Aggregate is Exact.Aggregate as of end: counts and sums over each flow's latest row, first /
// last / max over every row stored by then (AggregateFlows and TraceFlow).
func (y *History) Aggregate(end *int64, filters []ExactFilter) ([]ExactSummary, error) {
	n := len(filters)
	if n == 0 {
		return nil, nil
	}
	cf, err := exactFilters(filters)
	if err != nil {
		return nil, err
	}
	cs := make([]C.gns_ex_summary, n)
	if err := lastErr(C.gns_ex_hist_aggregate(y.h, endNs(end), &cf[0], C.uint32_t(n), &cs[0])); err != nil {
		return nil, err
	}
	return exactSummaries(cs), nil
}

// AggregateCIDR is Exact.AggregateCIDR as of end (gns_ex_hist_aggregate_cidr).
func (y *History) AggregateCIDR(end *int64, filters []ExactCIDR) ([]ExactSummary, error) {
	n := len(filters)
	if n == 0 {
		return nil, nil
	}
	cc, err := exactCIDRs(filters)
	if err != nil {
		return nil, err
	}
	cs := make([]C.gns_ex_summary, n)
	if err := lastErr(C.gns_ex_hist_aggregate_cidr(y.h, endNs(end), &cc[0], C.uint32_t(n), &cs[0])); err != nil {
		return nil, err
	}
	return exactSummaries(cs), nil
}

// HeavyHitters is Exact.HeavyHitters over each flow's latest row as of end (QueryHeavyHitters).
func (y *History) HeavyHitters(end *int64, metric int, threshold, limit uint64) (keys []byte, values []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_hist_heavy_hitters(y.h, endNs(end), C.int(metric), C.uint64_t(threshold), C.uint64_t(limit),
		nil, nil, &n)); err != nil || n == 0 {
		return nil, nil, err
	}
	m := int(n)
	keys, values = make([]byte, m*y.keyBytes+1), make([]uint64, m)
	err = lastErr(C.gns_ex_hist_heavy_hitters(y.h, endNs(end), C.int(metric), C.uint64_t(threshold), C.uint64_t(limit),
		(*C.uint8_t)(unsafe.Pointer(&keys[0])), (*C.uint64_t)(unsafe.Pointer(&values[0])), &n))
	if int(n) < m { // (an Append in between only adds rows; a shorter list cannot happen, but never read past it)
		m = int(n)
	}
	return keys[:m*y.keyBytes], values[:m], err
}

// Flows returns each flow's latest row as of end, in log order, in the layout of Exact.Flows.
func (y *History) Flows(end *int64) (keys []byte, start, last []int64, pkts, bytes []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_hist_snapshot(y.h, endNs(end), nil, nil, nil, nil, nil, &n)); err != nil {
		return
	}
	m := int(n)
	keys = make([]byte, m*y.keyBytes+1)
	start, last = make([]int64, m+1), make([]int64, m+1)
	pkts, bytes = make([]uint64, m+1), make([]uint64, m+1)
	err = lastErr(C.gns_ex_hist_snapshot(y.h, endNs(end), (*C.uint8_t)(unsafe.Pointer(&keys[0])),
		(*C.int64_t)(unsafe.Pointer(&start[0])), (*C.int64_t)(unsafe.Pointer(&last[0])),
		(*C.uint64_t)(unsafe.Pointer(&pkts[0])), (*C.uint64_t)(unsafe.Pointer(&bytes[0])), &n))
	if int(n) < m {
		m = int(n)
	}
	return keys[:m*y.keyBytes], start[:m], last[:m], pkts[:m], bytes[:m], err
}

// Trim expires the snapshots with timestamp < before (gns_ex_hist_trim).  fold keeps of them
// each flow's latest row as one base snapshot under the last expired timestamp, so answers at
// or after it are unchanged; without fold they are dropped with all their rows, as the
// reference drops a partition.  out: snapshots removed, rows released, keys forgotten, rows held.
func (y *History) Trim(before int64, fold bool) (out [4]uint64, err error) {
	f := C.int(0)
	if fold {
		f = 1
	}
	err = lastErr(C.gns_ex_hist_trim(y.h, C.int64_t(before), f, (*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return
}

// Export returns every log row in log order (gns_ex_hist_export) in the layout of Exact.Flows,
// with the number of the snapshot that wrote each row; Times gives the snapshots' timestamps.
func (y *History) Export() (keys []byte, start, last []int64, pkts, bytes []uint64, written []uint32, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_ex_hist_export(y.h, nil, nil, nil, nil, nil, nil, &n)); err != nil {
		return
	}
	m := int(n)
	keys = make([]byte, m*y.keyBytes+1)
	start, last = make([]int64, m+1), make([]int64, m+1)
	pkts, bytes = make([]uint64, m+1), make([]uint64, m+1)
	written = make([]uint32, m+1)
	err = lastErr(C.gns_ex_hist_export(y.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])),
		(*C.int64_t)(unsafe.Pointer(&start[0])), (*C.int64_t)(unsafe.Pointer(&last[0])),
		(*C.uint64_t)(unsafe.Pointer(&pkts[0])), (*C.uint64_t)(unsafe.Pointer(&bytes[0])),
		(*C.uint32_t)(unsafe.Pointer(&written[0])), &n))
	if int(n) < m {
		m = int(n)
	}
	return keys[:m*y.keyBytes], start[:m], last[:m], pkts[:m], bytes[:m], written[:m], err
}

// AppendRows stores one snapshot from host rows in the layout of Exact.Flows
// (gns_ex_hist_append_rows): every row carries packets and no key occurs twice.  No rows
// register the timestamp.  Feeding an empty history the rows Export gave, snapshot by
// snapshot, restores it.
func (y *History) AppendRows(keys []byte, start, last []int64, pkts, bytes []uint64, tsNano int64) (rows, newKeys uint64, err error) {
	n := len(pkts)
	if len(keys) != n*y.keyBytes || len(start) != n || len(last) != n || len(bytes) != n {
		return 0, 0, errors.New("sketchgpu: AppendRows: row slices differ in length")
	}
	var out [2]C.uint64_t
	if n == 0 {
		err = lastErr(C.gns_ex_hist_append_rows(y.h, nil, nil, nil, nil, nil, 0, C.int64_t(tsNano), &out[0]))
	} else {
		err = lastErr(C.gns_ex_hist_append_rows(y.h, (*C.uint8_t)(unsafe.Pointer(&keys[0])),
			(*C.int64_t)(unsafe.Pointer(&start[0])), (*C.int64_t)(unsafe.Pointer(&last[0])),
			(*C.uint64_t)(unsafe.Pointer(&pkts[0])), (*C.uint64_t)(unsafe.Pointer(&bytes[0])),
			C.uint64_t(n), C.int64_t(tsNano), &out[0]))
	}
	return uint64(out[0]), uint64(out[1]), err
}

// Close releases the history.
func (y *History) Close() { C.gns_ex_hist_destroy(y.h) }

// HeavyHistory is the store behind QueryHeavyHitters' EndTime for the sketch tasks
// (gns_hh_hist_*): it replaces the sketch ClickHouseWriter.Write (writer_clickhouse.go:86-138),
// which appends one row per list entry of each interval's Snapshot(), and the query over
// those rows (querier.go:191-248).  Append stores the lists of one interval as packed device
// rows [flow | u32] -- what View.HeavyRows and SuperSpreadView.HeavyRows write -- under a
// Timestamp; HeavyHitters answers, per flow, with the value of its latest row of one Type at
// or before an end time (nil: the newest snapshot).  A flow that left the list keeps its
// last listed value; one listed again supersedes its old row.  Calls may come from any
// goroutine.
type HeavyHistory struct {
	h        *C.gns_hh_hist
	keyBytes int
}

// HeavyList is one list of an interval: n packed device rows of keyBytes + 4 under a Type
// (0: Count-Min's count list, 1: its size list, 2: SuperSpread's list).
type HeavyList struct {
	Type uint32
	Rows unsafe.Pointer
	N    uint64
}

// NewHeavyHistory allocates a history for flows of keyBytes bytes.  maxRows and maxFlows are
// initial capacities (0: defaults); both grow.
func NewHeavyHistory(keyBytes int, maxRows, maxFlows uint64, device int) (*HeavyHistory, error) {
	var p C.gns_hh_hist_params
	p.key_bytes = C.uint32_t(keyBytes)
	p.max_rows, p.max_flows, p.device = C.uint64_t(maxRows), C.uint64_t(maxFlows), C.int(device)
	var h *C.gns_hh_hist
	if err := lastErr(C.gns_hh_hist_create(&p, &h)); err != nil {
		return nil, err
	}
	return &HeavyHistory{h: h, keyBytes: keyBytes}, nil
}

// Append stores the lists (device rows, at most one list per Type) as the next snapshot;
// tsNano must lie after the last one's.  No lists register the timestamp.
func (y *HeavyHistory) Append(tsNano int64, lists []HeavyList) (rows, newPairs uint64, err error) {
	var out [2]C.uint64_t
	cl := make([]C.gns_hh_list, len(lists)+1)
	for i, l := range lists {
		cl[i]._type = C.uint32_t(l.Type)
		cl[i].rows = (*C.uint8_t)(l.Rows)
		cl[i].n = C.uint64_t(l.N)
	}
	err = lastErr(C.gns_hh_hist_append(y.h, C.int64_t(tsNano), &cl[0], C.uint32_t(len(lists)), C.GNS_MEM_DEVICE, &out[0]))
	return uint64(out[0]), uint64(out[1]), err
}

// HeavyHitters lists the flows whose latest row of Type typ as of end has value >= threshold,
// value descending then flow bytes ascending, cut to limit rows when limit != 0.
func (y *HeavyHistory) HeavyHitters(end *int64, typ uint32, threshold, limit uint64) (flows []byte, values []uint64, err error) {
	var n C.uint64_t
	if err = lastErr(C.gns_hh_hist_heavy_hitters(y.h, endNs(end), C.uint32_t(typ), C.uint64_t(threshold), C.uint64_t(limit),
		nil, nil, &n)); err != nil || n == 0 {
		return nil, nil, err
	}
	m := int(n)
	flows, values = make([]byte, m*y.keyBytes+1), make([]uint64, m)
	err = lastErr(C.gns_hh_hist_heavy_hitters(y.h, endNs(end), C.uint32_t(typ), C.uint64_t(threshold), C.uint64_t(limit),
		(*C.uint8_t)(unsafe.Pointer(&flows[0])), (*C.uint64_t)(unsafe.Pointer(&values[0])), &n))
	if int(n) > m { // (an Append in between made the list longer: nothing was written)
		return nil, nil, fmt.Errorf("heavy history: the list grew from %d to %d rows between the calls", m, int(n))
	}
	m = int(n)
	return flows[:m*y.keyBytes], values[:m], err
}

// Times returns the snapshots' timestamps.
func (y *HeavyHistory) Times() ([]int64, error) {
	var n C.uint64_t
	if err := lastErr(C.gns_hh_hist_times(y.h, nil, &n)); err != nil || n == 0 {
		return nil, err
	}
	ts := make([]int64, int(n))
	err := lastErr(C.gns_hh_hist_times(y.h, (*C.int64_t)(unsafe.Pointer(&ts[0])), &n))
	if int(n) < len(ts) {
		ts = ts[:int(n)]
	}
	return ts, err
}

// Trim expires the snapshots with timestamp < before (gns_hh_hist_trim).  Without fold they are
// dropped with all their rows, as the reference drops a partition of heavy_hitters
// (writer_clickhouse.go:25-27): a (Type, flow) pair listed only in them is forgotten and the key
// index shrinks.  fold keeps of them, per Type, each flow's latest row as one base snapshot
// under the last expired timestamp, so answers at or after it are unchanged; it keeps one row per
// pair ever listed and never shrinks the index.  out: snapshots removed, rows removed, pairs
// forgotten, rows held.
func (y *HeavyHistory) Trim(before int64, fold bool) (out [4]uint64, err error) {
	f := C.int(0)
	if fold {
		f = 1
	}
	err = lastErr(C.gns_hh_hist_trim(y.h, C.int64_t(before), f, (*C.uint64_t)(unsafe.Pointer(&out[0]))))
	return
}

// Query answers, for each of the len(flows)/keyBytes flows, with the value of its latest row of
// Type typ as of end (gns_hh_hist_query); found[i] is false, and the value 0, for a flow without
// such a row.  Nothing is inserted.
func (y *HeavyHistory) Query(end *int64, typ uint32, flows []byte) (values []uint64, found []bool, err error) {
	if len(flows)%y.keyBytes != 0 {
		return nil, nil, errors.New("sketchgpu: Query: flows is not a multiple of the key width")
	}
	n := len(flows) / y.keyBytes
	if n == 0 {
		return nil, nil, nil
	}
	values = make([]uint64, n)
	f8 := make([]uint8, n)
	err = lastErr(C.gns_hh_hist_query(y.h, endNs(end), C.uint32_t(typ), (*C.uint8_t)(unsafe.Pointer(&flows[0])), C.uint64_t(n),
		C.GNS_MEM_HOST, (*C.uint64_t)(unsafe.Pointer(&values[0])), (*C.uint8_t)(unsafe.Pointer(&f8[0]))))
	found = make([]bool, n)
	for i, b := range f8 {
		found[i] = b != 0
	}
	return
}

// Close releases the history.
func (y *HeavyHistory) Close() { C.gns_hh_hist_destroy(y.h) }

// ThriftDecoder holds the device buffers one batch of NATS messages decodes into
// (ns-engine's live path: stream_aggregator.go:85 decodes one PacketInfo message
// at a time with probe.UnmarshalPacketInfo, packetcodec.go:97-108; here a whole
// batch is decoded on the GPU into the engine's pre-parsed records).
type ThriftDecoder struct {
	rec, wirelen, ts unsafe.Pointer
	capacity         int
	device           int
}

// NewThriftDecoder allocates room for `capacity` messages per batch on `device`.
func NewThriftDecoder(capacity, device int) (*ThriftDecoder, error) {
	d := &ThriftDecoder{capacity: capacity, device: device}
	for _, b := range []struct {
		p     *unsafe.Pointer
		bytes int
	}{{&d.rec, 64 * capacity}, {&d.wirelen, 4 * capacity}, {&d.ts, 8 * capacity}} {
		if err := lastErr(C.gns_device_alloc(C.uint64_t(b.bytes), C.int(device), b.p)); err != nil {
			d.Close()
			return nil, err
		}
	}
	return d, nil
}

// decode turns msgs (back to back; offs[i] = start of message i, offs[n] = len(msgs))
// into device records; bad counts the messages the reference would reject.
func (d *ThriftDecoder) decode(msgs []byte, offs []uint64) (n int, bad uint64, err error) {
	n = len(offs) - 1
	if n <= 0 {
		return 0, 0, nil
	}
	if n > d.capacity {
		return 0, 0, fmt.Errorf("sketchgpu: %d messages for a %d-message decoder", n, d.capacity)
	}
	var nb C.uint64_t
	err = lastErr(C.gns_thrift_decode((*C.uint8_t)(unsafe.Pointer(&msgs[0])), C.uint64_t(len(msgs)),
		(*C.uint64_t)(unsafe.Pointer(&offs[0])), C.uint64_t(n), (*C.uint8_t)(d.rec), (*C.uint32_t)(d.wirelen),
		(*C.int64_t)(d.ts), &nb, C.GNS_MEM_HOST, C.int(d.device)))
	return n, uint64(nb), err
}

// Close frees the device buffers.
func (d *ThriftDecoder) Close() {
	for _, p := range []unsafe.Pointer{d.rec, d.wirelen, d.ts} {
		if p != nil {
			C.gns_device_free(p, C.int(d.device))
		}
	}
	d.rec, d.wirelen, d.ts = nil, nil, nil
}

// InsertThriftBatch decodes a batch of PacketInfo messages on the GPU and inserts
// the packets (ProcessPacket for each message, task.go:156-169).  It returns once
// the decoder's buffers are free again.
func (c *CountMin) InsertThriftBatch(d *ThriftDecoder, msgs []byte, offs []uint64) (bad uint64, err error) {
	n, bad, err := d.decode(msgs, offs)
	if err != nil || n == 0 {
		return bad, err
	}
	if err = lastErr(C.gns_cm_insert_headers(c.h, (*C.uint8_t)(d.rec), (*C.uint32_t)(d.wirelen), C.uint64_t(n),
		C.GNS_MEM_DEVICE)); err != nil {
		return bad, err
	}
	return bad, lastErr(C.gns_cm_flush(c.h))
}

// InsertThriftBatch for SuperSpread (see CountMin.InsertThriftBatch).
func (s *SuperSpread) InsertThriftBatch(d *ThriftDecoder, msgs []byte, offs []uint64) (bad uint64, err error) {
	n, bad, err := d.decode(msgs, offs)
	if err != nil || n == 0 {
		return bad, err
	}
	if err = lastErr(C.gns_ss_insert_headers(s.h, (*C.uint8_t)(d.rec), (*C.uint32_t)(d.wirelen), C.uint64_t(n),
		C.GNS_MEM_DEVICE)); err != nil {
		return bad, err
	}
	return bad, lastErr(C.gns_ss_flush(s.h))
}

// InsertThriftBatch for the exact aggregator (the messages' TimestampUnixNano kept).
func (e *Exact) InsertThriftBatch(d *ThriftDecoder, msgs []byte, offs []uint64) (bad uint64, err error) {
	n, bad, err := d.decode(msgs, offs)
	if err != nil || n == 0 {
		return bad, err
	}
	if err = lastErr(C.gns_ex_insert_headers(e.h, (*C.uint8_t)(d.rec), (*C.uint32_t)(d.wirelen), (*C.int64_t)(d.ts),
		C.uint64_t(n), C.GNS_MEM_DEVICE)); err != nil {
		return bad, err
	}
	return bad, lastErr(C.gns_ex_flush(e.h))
}
