// gns_common.cpp -- host plumbing (see gns_common.hpp).
#include "gns_common.hpp"

#include <chrono>
#include <mutex>

namespace gns {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int dalloc(void **p, size_t bytes) {
    *p = nullptr;
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        *p = nullptr;
        return GNS_E_OOM;
    }
    return GNS_OK;
}

void dfree(void *p) {
    if (p) (void)hipFree(p);
}

int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available");
        return GNS_E_NODEV;
    }
    if (device < 0 || device >= ndev) { set_error("device %d out of range", device); return GNS_E_ARG; }
    return GNS_OK;
}

int set_device(int device) {
    (void)hipGetLastError();
    GNS_HIP(hipSetDevice(device));
    return GNS_OK;
}

int stream_wait_now(hipStream_t waiter, hipStream_t on, const char *what) {
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) {
        e = hipEventRecord(ev, on);
        if (e == hipSuccess) e = hipStreamWaitEvent(waiter, ev, 0);
        (void)hipEventDestroy(ev);  // the wait is queued: the runtime keeps what it needs
    }
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return GNS_E_HIP; }
    return GNS_OK;
}

uint64_t test_piece(const char *env_name, uint64_t dflt) {
    const char *env = getenv(env_name);
    const unsigned long long v = env ? strtoull(env, nullptr, 10) : 0;
    return v ? std::min<uint64_t>(v, dflt) : dflt;
}

InputDesc advance(const InputDesc &in, uint64_t off) {
    InputDesc d = in;
    if (d.hdr) d.hdr += off * 16;
    if (d.src16) d.src16 += off * 16;
    if (d.dst16) d.dst16 += off * 16;
    if (d.sport) d.sport += off;
    if (d.dport) d.dport += off;
    if (d.proto) d.proto += off;
    if (d.keys) d.keys += off * d.stride;
    if (d.keys2) d.keys2 += off * d.stride2;
    if (d.rec16) d.rec16 += off * 4;
    if (d.sizes) d.sizes += off;
    return d;
}

void stage_input(StageList &l, InputDesc &d, uint64_t m) {
    stage_add(l, d.hdr, d.hdr ? m * 64 : 0, &d.hdr);
    stage_add(l, d.src16, d.src16 ? m * 16 : 0, &d.src16);
    stage_add(l, d.dst16, d.dst16 ? m * 16 : 0, &d.dst16);
    stage_add(l, d.sport, d.sport ? m * 2 : 0, &d.sport);
    stage_add(l, d.dport, d.dport ? m * 2 : 0, &d.dport);
    stage_add(l, d.proto, d.proto ? m : 0, &d.proto);
    stage_add(l, d.keys, d.keys ? m * d.stride : 0, &d.keys);
    stage_add(l, d.keys2, d.keys2 ? m * d.stride2 : 0, &d.keys2);
    stage_add(l, d.rec16, d.rec16 ? m * 16 : 0, &d.rec16);
    stage_add(l, d.sizes, d.sizes ? m * 4 : 0, &d.sizes);
}

size_t HostStage::need(const StageList &l) {
    size_t tot = 0;
    for (const StageItem &it : l) tot += (it.bytes + 15) & ~size_t(15);
    return tot;
}

int HostStage::copy(const StageList &l, hipStream_t s) {
    const size_t tot = need(l);
    if (cap < tot) {
        free_all();
        GNS_TRY(dalloc(reinterpret_cast<void **>(&buf), tot));
        cap = tot;
    }
    uint8_t *p = buf;
    for (const StageItem &it : l) {
        if (!it.bytes) continue;
        if (it.src) GNS_HIP(hipMemcpyAsync(p, it.src, it.bytes, hipMemcpyHostToDevice, s));
        *it.patch = p;
        p += (it.bytes + 15) & ~size_t(15);
    }
    return GNS_OK;
}

void HostStage::free_all() {
    dfree(buf);
    buf = nullptr;
    cap = 0;
}

void FlowDict::limits() {
    D.cap = (uint32_t)(dict_slots - dict_slots / 4);
    max_flows = std::max<uint64_t>(max_flows, dict_slots / 2);
}

int FlowDict::reclaim(DictIds *ids, int n, uint64_t min_slots, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t before = claimed, slots0 = dict_slots;
    uint64_t live = 0;
    GNS_TRY(dict_rebuild(D, dict_slots, ids, n, nullptr, ids, n, std::min(kDictMaxSlots, std::max(dict_slots, min_slots)),
                         s, dsc, &live, nullptr, kDictMaxSlots));
    reclaim_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    n_reclaim++;
    if (dict_slots != slots0) n_grow++;
    limits();
    n_dropped += before > live ? before - live : 0;
    claimed = live;
    last_live = live;
    return GNS_OK;
}

void FlowDict::stats(uint64_t out[8]) const {
    out[0] = n_reclaim; out[1] = n_dropped; out[2] = last_live; out[3] = claimed;
    out[4] = (uint64_t)(reclaim_ms * 1000.0); out[5] = n_retry;
    out[6] = dict_slots; out[7] = n_grow;
}

void FlowDict::free_all() {
    dfree(D.rec); dfree(dctl); dfree(stats_bak);
    dsc.free_all();
}

int PinnedOut::reserve(size_t bytes) {
    for (hipEvent_t &e : ev)
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            set_error("view event");
            return GNS_E_HIP;
        }
    if (bytes <= pin_n && pin) return GNS_OK;
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    pin_n = 0;
    const size_t want = std::max<size_t>(2 * bytes, 2 * kPinChunk);
    if (hipHostMalloc(reinterpret_cast<void **>(&pin), want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipHostMalloc(%zu bytes) failed", want);
        return GNS_E_OOM;
    }
    pin_n = want;
    return GNS_OK;
}

int PinnedOut::copy_out(void *dst, const void *src, size_t bytes, hipStream_t s, size_t sw, size_t dw) {
    const size_t piece = pin_piece(kPinChunk, sw), n = pin_pieces(bytes, piece);
    for (size_t j = 0; j <= n; j++) {
        if (j < n) {
            GNS_HIP(hipMemcpyAsync(pin + (j & 1) * kPinChunk, static_cast<const uint8_t *>(src) + pin_off(j, piece),
                                   pin_len(j, piece, bytes), hipMemcpyDeviceToHost, s));
            GNS_HIP(hipEventRecord(ev[j & 1], s));
        }
        if (j > 0) {
            GNS_HIP(hipEventSynchronize(ev[(j - 1) & 1]));
            pin_land(static_cast<uint8_t *>(dst), pin + ((j - 1) & 1) * kPinChunk, j - 1, piece, bytes, sw, dw);
        }
    }
    return GNS_OK;
}

int PinnedOut::copy_in(void *dst, const void *src, size_t bytes, hipStream_t s) {
    int half = 0;
    for (size_t off = 0; off < bytes; off += kPinChunk, half ^= 1) {
        const size_t m = std::min(kPinChunk, bytes - off);
        uint8_t *p = pin + (size_t)half * kPinChunk;
        if (off >= 2 * kPinChunk) GNS_HIP(hipEventSynchronize(ev[half]));  // the half's last copy has landed
        memcpy(p, static_cast<const uint8_t *>(src) + off, m);
        GNS_HIP(hipMemcpyAsync(static_cast<uint8_t *>(dst) + off, p, m, hipMemcpyHostToDevice, s));
        GNS_HIP(hipEventRecord(ev[half], s));
    }
    GNS_HIP(hipStreamSynchronize(s));
    return GNS_OK;
}

void PinnedOut::free_all() {
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    pin_n = 0;
    for (hipEvent_t &e : ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

void QueryStage::free_all() {
    dfree(qkeys); dfree(qout);
    qkeys = nullptr; qout = nullptr;
    qkeys_n = qout_n = 0;
}

int query_keys(int device, hipStream_t s, QueryStage &st, const char *what, const uint8_t *keys, uint32_t stride,
               uint32_t key_bytes, uint64_t n, uint64_t *out, bool dev, const LaunchFn &launch) {
    if (n && (!keys || !out)) { set_error("null argument"); return GNS_E_ARG; }
    if (n == 0) return GNS_OK;
    if (stride < key_bytes) { set_error("%s query: stride %u < key bytes %u", what, stride, key_bytes); return GNS_E_ARG; }
    if (dev && ((uintptr_t)out & 7u) != 0) { set_error("answers not 8-byte aligned"); return GNS_E_ARG; }
    GNS_TRY(set_device(device));
    const size_t kb = (size_t)n * stride, ob = (size_t)n * 8, koff = (ob + 15) & ~(size_t)15;
    const uint8_t *hk = keys;  // what the copies read and write: the caller's memory, or the pinned
    uint64_t *ho = out;        // staging {answers, keys at koff}
    if (!dev) {
        GNS_TRY(grow_buf(&st.qkeys, st.qkeys_n, (uint64_t)kb));
        GNS_TRY(grow_buf(&st.qout, st.qout_n, n));
        if (st.pin) {
            GNS_TRY(st.pin->reserve(koff + kb));
            memcpy(st.pin->pin + koff, keys, kb);
            hk = st.pin->pin + koff;
            ho = reinterpret_cast<uint64_t *>(st.pin->pin);
        }
    }
    hipError_t e = dev ? hipSuccess : hipMemcpyAsync(st.qkeys, hk, kb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        const int rc = launch(dev ? keys : st.qkeys, dev ? out : st.qout);
        if (rc != GNS_OK) {  // (a view that cannot answer) the key copy may not outlive the caller's array
            (void)hipStreamSynchronize(s);
            return rc;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess && !dev) e = hipMemcpyAsync(ho, st.qout, ob, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_error("%s query: %s", what, hipGetErrorString(e)); return GNS_E_HIP; }
    if (ho != out) memcpy(out, ho, ob);
    return GNS_OK;
}

int ViewCore::init() {
    int lo_pri = 0, hi_pri = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);
    if (hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, hi_pri) != hipSuccess ||
        hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        set_error("view stream/event");
        return GNS_E_HIP;
    }
    return GNS_OK;
}

int ViewCore::publish(hipStream_t handle_stream) {
    GNS_HIP(hipEventRecord(ready, handle_stream));
    GNS_HIP(hipStreamWaitEvent(stream, ready, 0));
    return GNS_OK;
}

void ViewCore::quiesce() {
    std::lock_guard<std::mutex> lk(mu);
    if (stream) (void)hipStreamSynchronize(stream);
}

void ViewCore::destroy() {
    if (ready) (void)hipEventDestroy(ready);
    if (stream) (void)hipStreamDestroy(stream);
    ready = nullptr;
    stream = nullptr;
}

int stats_save(unsigned long long *bak, const unsigned long long *stats, hipStream_t s) {
    GNS_HIP(hipMemcpyAsync(bak, stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    return GNS_OK;
}

int stats_undo(unsigned long long *stats, const unsigned long long *bak, bool clear_full, hipStream_t s) {
    GNS_HIP(hipMemcpyAsync(stats, bak, 3 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    if (clear_full) GNS_HIP(hipMemsetAsync(stats + 3, 0, sizeof(unsigned long long), s));
    return GNS_OK;
}

int DictRecovery::batch(const InputDesc &d, uint64_t m, bool fresh) const {
    if (m == 0) return GNS_OK;
    if (fd.full) {
        set_error("flow dictionary full (%llu slots, %llu live flows)", (unsigned long long)fd.dict_slots,
                  (unsigned long long)fd.last_live);
        return GNS_E_FULL;
    }
    if (fd.claimed >= fd.max_flows) {  // proactive: keep the load <= ~1/2
        GNS_TRY(reclaim(0));
        fresh = true;
    }
    for (;;) {
        GNS_TRY(stats_save(fd.stats_bak, stats, stream));
        const int rc = run(d, m);
        // (full: a piece of a split made by run itself has already failed for good)
        if (rc != GNS_E_FULL || fd.full) return rc;
        // not applied: undo its counters, drop its claims and the dead flows
        GNS_TRY(stats_undo(stats, fd.stats_bak, true, stream));
        fd.n_retry++;
        if (!fresh) {  // the flows that died since the last rebuild may be room enough
            GNS_TRY(reclaim(0));
            fresh = true;
            continue;
        }
        if (m > chunk) {  // split: each half meets a fresh dictionary
            GNS_TRY(reclaim(0));
            break;
        }
        if (fd.dict_slots >= kDictMaxSlots) {  // cannot happen below ~ 3/4 * 2^30 live flows
            GNS_TRY(reclaim(0));
            fd.full = true;
            const unsigned long long one = 1;
            GNS_HIP(hipMemcpy(stats + 3, &one, sizeof(one), hipMemcpyHostToDevice));
            set_error("flow dictionary full: %llu live flows plus one %s exceed %llu slots",
                      (unsigned long long)fd.last_live, piece, (unsigned long long)fd.dict_slots);
            return GNS_E_FULL;
        }
        GNS_TRY(reclaim(fd.dict_slots * 2));  // grow, then re-run the piece
    }
    const uint64_t h = ((m / 2 + chunk - 1) / chunk) * chunk;
    GNS_TRY(batch(d, h, true));
    return batch(advance(d, h), m - h, false);
}

uint32_t layout_bytes(const gns_layout &l) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < l.n_fields && i < 8; i++) {
        switch (l.fields[i]) {
        case GNS_F_SRCIP: case GNS_F_DSTIP: k += 16; break;
        case GNS_F_SRCPORT: case GNS_F_DSTPORT: k += 2; break;
        case GNS_F_PROTO: k += 1; break;
        default: break;  // unknown field names contribute nothing (task.go:335-336)
        }
    }
    return k;
}

int make_plan(const gns_layout &l, uint32_t key_bytes, KeyPlanN *kp) {
    memset(kp, 0, sizeof(*kp));
    if (l.n_fields > 8) { set_error("layout has %u fields (max 8)", l.n_fields); return GNS_E_ARG; }
    const uint32_t K = l.n_fields ? layout_bytes(l) : key_bytes;
    if (K > 37) {  // task.go:74: the pooled key buffer is 37 bytes; Go panics beyond
        set_error("flow key of %u bytes exceeds the reference maximum of 37", K);
        return GNS_E_ARG;
    }
    if (l.n_fields && key_bytes && key_bytes != K) {
        set_error("key_bytes=%u disagrees with the layout's %u bytes", key_bytes, K);
        return GNS_E_ARG;
    }
    kp->K = K;
    // tuple byte index of every key byte
    uint32_t off = 0;
    for (uint32_t i = 0; i < l.n_fields; i++) {
        uint32_t base = 0, len = 0;
        switch (l.fields[i]) {
        case GNS_F_SRCIP: base = 0; len = 16; break;
        case GNS_F_DSTIP: base = 16; len = 16; break;
        case GNS_F_SRCPORT: base = 32; len = 2; break;
        case GNS_F_DSTPORT: base = 34; len = 2; break;
        case GNS_F_PROTO: base = 36; len = 1; break;
        default: break;
        }
        for (uint32_t j = 0; j < len; j++) kp->src[off + j] = (uint8_t)(base + j);
        off += len;
    }
    for (uint32_t j = off; j < 80; j++) kp->src[j] = 255;
    // SLICE fast path: key == tuple bytes [4*woff, 4*woff+K)
    kp->woff = -1;
    for (int woff : {0, 4}) {
        bool ok = K > 0;
        for (uint32_t j = 0; j < K && ok; j++) ok = kp->src[j] == (uint8_t)(4 * woff + j);
        if (ok) { kp->woff = woff; break; }
    }
    return GNS_OK;
}

int make_plan2(const gns_layout &a, const gns_layout &b, KeyPlanN *kp) {
    KeyPlanN pa, pb;
    GNS_TRY(make_plan(a, 0, &pa));
    GNS_TRY(make_plan(b, 0, &pb));
    memset(kp, 0, sizeof(*kp));
    kp->K = pa.K + pb.K;
    for (uint32_t j = 0; j < 80; j++) kp->src[j] = 255;
    for (uint32_t j = 0; j < pa.K; j++) kp->src[j] = pa.src[j];
    for (uint32_t j = 0; j < pb.K; j++) kp->src[pa.K + j] = pb.src[j];
    kp->woff = -1;
    for (int woff : {0, 4}) {
        bool ok = kp->K > 0;
        for (uint32_t j = 0; j < kp->K && ok; j++) ok = kp->src[j] == (uint8_t)(4 * woff + j);
        if (ok) { kp->woff = woff; break; }
    }
    return GNS_OK;
}

hipEvent_t StageTimer::get() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void StageTimer::begin(int stage, hipEvent_t *a) {
    *a = nullptr;
    if (!on || !((mask >> stage) & 1u)) return;
    *a = get();
    if (*a) (void)hipEventRecord(*a, stream);
}

void StageTimer::end(int stage, hipEvent_t a) {
    if (!on || !a) return;
    hipEvent_t b = get();
    if (!b) return;
    (void)hipEventRecord(b, stream);
    pending.push_back({a, b, stage});
}

int StageTimer::collect() {
    for (auto &p : pending) {
        (void)hipEventSynchronize(p.b);
        float t = 0.f;
        if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
            ms[p.stage] += t;
            launches[p.stage] += 1;
        }
        pool.push_back(p.a);
        pool.push_back(p.b);
    }
    pending.clear();
    return GNS_OK;
}

void StageTimer::report(double *ms_out, uint64_t *launches_out, int reset) {
    collect();
    for (int i = 0; i < kStages; i++) {
        if (ms_out) ms_out[i] = ms[i];
        if (launches_out) launches_out[i] = launches[i];
        if (reset) { ms[i] = 0; launches[i] = 0; }
    }
}

int handle_flush(int device, hipStream_t stream, StageTimer &timer) {
    GNS_TRY(set_device(device));
    GNS_HIP(hipStreamSynchronize(stream));
    timer.collect();
    return GNS_OK;
}

void StageTimer::destroy() {
    collect();
    for (auto e : pool) (void)hipEventDestroy(e);
    pool.clear();
}

void default_seeds(uint32_t *out, uint32_t n) {
    uint64_t s = 0x9747B28Cull;
    for (uint32_t i = 0; i < n; i++) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        out[i] = (uint32_t)(z ^ (z >> 31));
    }
}

}  // namespace gns

extern "C" int gns_device_alloc(uint64_t bytes, int device, void **out) {
    if (!out) { gns::set_error("null argument"); return GNS_E_ARG; }
    *out = nullptr;
    (void)hipGetLastError();
    GNS_TRY(gns::check_device(device));
    if (hipSetDevice(device) != hipSuccess) { gns::set_error("hipSetDevice(%d) failed", device); return GNS_E_HIP; }
    return gns::dalloc(out, bytes);
}

extern "C" int gns_device_free(void *p, int device) {
    if (!p) return GNS_OK;
    if (hipSetDevice(device) != hipSuccess) { gns::set_error("hipSetDevice(%d) failed", device); return GNS_E_HIP; }
    return hipFree(p) == hipSuccess ? GNS_OK : GNS_E_HIP;
}

extern "C" const char *gns_last_error(void) { return gns::g_last_error.c_str(); }
extern "C" const char *gns_version(void) { return "gns-sketch 0.1 (gfx950)"; }
