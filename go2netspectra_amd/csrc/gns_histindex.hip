// gns_histindex.hip -- HistIndex (gns_histindex.hpp): the key index both histories share.
//   k_hi_heads    the slots a head array names name themselves in dict_rebuild's mark list
//   k_hi_permute  a head word follows its record to the slot a rebuild gave it (gns_dict.hip remap)
//   k_hi_own / k_hi_dup  no two rows in one index slot
#include "gns_histindex.hpp"

namespace gns {

namespace {
unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

// a slot claimed by an append that did not complete names nothing and is dropped (ids: cleared
// to GNS_ID_NONE before the first head array)
__global__ __launch_bounds__(256) void k_hi_heads(const uint32_t *head, uint64_t slots, uint32_t *ids) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < slots && head[s] != kHistOpen) ids[s] = (uint32_t)s;
}
__global__ __launch_bounds__(256) void k_hi_permute(const uint32_t *oh, uint64_t slots, const uint32_t *remap, uint32_t *nh) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const uint32_t t = remap[s];
    if (t >= kDictMarked) return;
    nh[t] = oh[s];
}
// Two rows of one call with one key would share a head word, which the link must not meet: every
// row names itself in its slot's owner word, and a row that then reads another's name there is a
// duplicate (one of the equal rows wins the word, every other one sees it).
__global__ __launch_bounds__(256) void k_hi_own(const uint32_t *ids, uint64_t n, uint32_t slots, uint32_t *owner) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    if (id < slots) owner[id] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_hi_dup(const uint32_t *ids, uint64_t n, uint32_t slots, const uint32_t *owner,
                                                uint32_t *dup) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const uint32_t id = ids[i];
        bad = id >= slots || owner[id] != (uint32_t)i;
    }
    if (bad) *dup = 1u;  // (every writer stores the same word)
}
}  // namespace

int HistIndex::init(const char *what_, uint32_t K, uint64_t slots_, hipStream_t s) {
    what = what_;
    slots = slots_;
    D.mask = (uint32_t)(slots - 1);
    D.K = K;
    D.RW = dict_record_words(K);
    D.seed = 0x5BD1E995u;
    D.cap = (uint32_t)(slots - slots / 4);
    GNS_TRY(dalloc_t(&D.rec, slots * D.RW));
    GNS_TRY(dalloc_t(&dctl, 4));
    GNS_TRY(dalloc_t(&full, 1));
    GNS_TRY(dalloc_t(&fresh, 4));
    D.ctl = dctl;
    if (hipMemsetAsync(D.rec, 0, slots * D.RW * 4, s) != hipSuccess || hipMemsetAsync(dctl, 0, 16, s) != hipSuccess ||
        hipMemsetAsync(full, 0, 8, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s create: device clear failed", what);
        return GNS_E_HIP;
    }
    return GNS_OK;
}

void HistIndex::free_all() {
    dfree(D.rec); dfree(dctl); dfree(full); dfree(ids); dfree(mark); dfree(fresh);
    dsc.free_all();
    rsc.free_all();
}

hipError_t HistIndex::queue_marks(const uint32_t *const *heads, size_t nheads, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(mark, 0xFF, slots * 4, s);  // GNS_ID_NONE
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < nheads; i++) hipLaunchKernelGGL(k_hi_heads, dim3(grid256(slots)), dim3(256), 0, s, heads[i], slots, mark);
    return hipGetLastError();
}

void HistIndex::permute(const uint32_t *oh, uint64_t old_slots, uint32_t *nh, hipStream_t s) const {
    hipLaunchKernelGGL(k_hi_permute, dim3(grid256(old_slots)), dim3(256), 0, s, oh, old_slots, (const uint32_t *)dsc.remap, nh);
}

int HistIndex::grow(uint64_t want, uint64_t done, const std::vector<uint32_t **> &heads, hipStream_t s,
                    const AfterRemap &after_remap) {
    const uint64_t old_slots = slots, new_slots = grown(want);
    if (new_slots > kDictMaxSlots) {
        set_error("%s key index cannot grow beyond 2^30 slots", what);
        return GNS_E_FULL;
    }
    GNS_TRY(reserve_mark(new_slots));
    std::vector<uint32_t *> oh(heads.size()), nh(heads.size(), nullptr);
    auto drop = [&]() { for (uint32_t *p : nh) dfree(p); };
    int rc = GNS_OK;
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < nh.size() && rc == GNS_OK && e == hipSuccess; i++) {
        oh[i] = *heads[i];
        if ((rc = dalloc_t(&nh[i], new_slots)) == GNS_OK) e = hipMemsetAsync(nh[i], 0xFF, new_slots * 4, s);
    }
    if (rc == GNS_OK && e == hipSuccess) e = queue_marks(oh.data(), oh.size(), s);
    if (rc == GNS_OK && e != hipSuccess) { set_error("%s index growth: %s", what, hipGetErrorString(e)); rc = GNS_E_HIP; }
    if (rc != GNS_OK) { drop(); return rc; }
    DictIds marks[2] = {{mark, old_slots}, {ids, done}};
    DictIds remaps[1] = {{ids, done}};
    uint64_t live = 0;
    rc = dict_rebuild(D, slots, marks, 2, nullptr, remaps, 1, new_slots, s, dsc, &live, nullptr);
    if (rc != GNS_OK) { drop(); return rc; }
    for (size_t i = 0; i < nh.size(); i++) permute(oh[i], old_slots, nh[i], s);
    if (after_remap) after_remap(dsc.remap, old_slots);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    // (the table is the new one whatever the kernels did: the old head words no longer fit it)
    for (size_t i = 0; i < nh.size(); i++) {
        dfree(oh[i]);
        *heads[i] = nh[i];
    }
    D.cap = (uint32_t)(slots - slots / 4);
    claimed = live;
    n_index_grow++;
    if (e != hipSuccess) { set_error("%s index growth: %s", what, hipGetErrorString(e)); return GNS_E_HIP; }
    return GNS_OK;
}

int HistIndex::resolve(const uint8_t *keys, uint32_t stride, uint64_t n, uint64_t at, hipStream_t s, const GrowFn &grow_fn) {
    for (uint64_t off = 0; off < n; off += kResolvePiece) {
        const uint64_t m = std::min<uint64_t>(kResolvePiece, n - off);
        if (claimed >= slots / 2) GNS_TRY(grow_fn(0, at + off));
        KeyResolve r{};
        r.keys = keys + off * stride;
        r.stride = stride; r.n = m; r.live = KEYS_ALL; r.vals = nullptr; r.ids = ids + at + off;
        r.full_word = full;
        for (;;) {
            const int rc = dict_resolve_keys(D, epoch, r, rsc, s, &claimed, nullptr, 0);
            if (rc != GNS_E_FULL) { GNS_TRY(rc); break; }
            GNS_HIP(hipMemsetAsync(full, 0, sizeof(unsigned long long), s));
            GNS_TRY(grow_fn(m, at + off));
        }
    }
    return GNS_OK;
}

int HistIndex::own(const uint32_t *ids_, uint64_t n, hipStream_t s) {
    GNS_TRY(reserve_mark(slots));
    hipLaunchKernelGGL(k_hi_own, dim3(grid256(n)), dim3(256), 0, s, ids_, n, (uint32_t)slots, mark);
    return GNS_OK;
}

int HistIndex::check_unique(const uint32_t *ids_, uint64_t n, uint32_t *flag, hipStream_t s) {
    GNS_TRY(own(ids_, n, s));
    hipLaunchKernelGGL(k_hi_dup, dim3(grid256(n)), dim3(256), 0, s, ids_, n, (uint32_t)slots, (const uint32_t *)mark, flag);
    GNS_HIP(hipGetLastError());
    return GNS_OK;
}

int HistIndex::shrink_beside(uint64_t want, hipStream_t s) {
    Dn = D;
    slots_n = slots;
    live_n = claimed;
    old_rec = nullptr;
    DictIds marks[1] = {{mark, slots}};
    ctl_touched = true;
    GNS_TRY(dict_rebuild(Dn, slots_n, marks, 1, nullptr, nullptr, 0, want, s, dsc, &live_n, &old_rec, 0, true));
    rebuilt = true;
    return GNS_OK;
}

void HistIndex::commit() {
    if (rebuilt) {
        dfree(old_rec);
        D = Dn;
        slots = slots_n;
        D.cap = (uint32_t)(slots - slots / 4);
        claimed = live_n;
    }
    rebuilt = ctl_touched = false;
}

void HistIndex::rollback() {
    if (rebuilt) dfree(Dn.rec);
    if (ctl_touched) {
        const uint32_t ctl[2] = {(uint32_t)claimed, 0u};
        (void)hipMemcpy(dctl, ctl, 8, hipMemcpyHostToDevice);
    }
    rebuilt = ctl_touched = false;
}

}  // namespace gns
