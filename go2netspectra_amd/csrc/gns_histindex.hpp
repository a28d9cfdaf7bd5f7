// gns_histindex.hpp -- the key index of a history (gns_ex_hist_*, gns_hh_hist_*): a dictionary of
// the store's own (gns_dict.hip) whose slots the store's head words are numbered by, with the
// growth that renumbers them, the piece-by-piece resolve of an append's keys, the "no two rows in
// one slot" check, and the rebuild a trim runs beside the live table.  Which slots survive a trim
// and what a head word holds stay the store's.  Kernels: gns_histindex.hip.
// Internal: not part of the C ABI.
#pragma once
#include <functional>
#include <vector>

#include "gns_common.hpp"
#include "gns_histplan.hpp"

namespace gns {

struct HistIndex {
    const char *what = "history";  // the store's word in error messages
    DictDev D{};
    uint64_t slots = 0, claimed = 0;
    uint32_t *dctl = nullptr;
    unsigned long long *full = nullptr;  // the dictionary-full word
    uint32_t epoch = 0;
    DictScratch dsc;
    KeyResolveScratch rsc;
    uint32_t *ids = nullptr;   // the index slots of the rows being appended
    uint64_t ids_n = 0;
    uint32_t *mark = nullptr;  // [slots] mark_heads' list (dict_rebuild's mark list), own()'s owner words
    uint64_t mark_n = 0;
    uint32_t *fresh = nullptr;  // [0] keys the running append added, [1] its duplicate flag
    uint64_t n_index_grow = 0;

    // An empty table of `slots` slots for K-byte keys, cleared on s.  Synchronizes s.
    int init(const char *what, uint32_t K, uint64_t slots, hipStream_t s);
    void free_all();
    int reserve_mark(uint64_t n) { return mark_n < n ? grow_buf(&mark, mark_n, n) : GNS_OK; }

    // mark[slot] = slot for every slot some head array names, GNS_ID_NONE for the others
    int mark_heads(const uint32_t *const *heads, size_t nheads, hipStream_t s) {
        GNS_TRY(reserve_mark(slots));
        GNS_HIP(queue_marks(heads, nheads, s));
        return GNS_OK;
    }
    // nh[remap[slot]] = oh[slot] over the slots the last rebuild kept (nh: cleared to kHistOpen)
    void permute(const uint32_t *oh, uint64_t old_slots, uint32_t *nh, hipStream_t s) const;

    // The index rebuilt into at least `want` slots (at least twice as many as now).  Kept: the
    // slots some head array names and the `done` ids the running append has resolved, which
    // are renumbered; claims of a piece that overflowed, and of appends that were rejected, are
    // dropped.  Every head array is replaced by one that follows the records; after_remap runs
    // before the stream is synchronized (what else is numbered by slot).  After a failed kernel
    // the index and the head arrays are still the new, mutually consistent ones.
    using AfterRemap = std::function<void(const uint32_t *remap, uint64_t old_slots)>;
    int grow(uint64_t want, uint64_t done, const std::vector<uint32_t **> &heads, hipStream_t s,
             const AfterRemap &after_remap = nullptr);
    // the slots grow(want) gives; beyond kDictMaxSlots it refuses with GNS_E_FULL
    uint64_t grown(uint64_t want) const {
        uint64_t n = slots * 2;
        while (n < want) n *= 2;
        return n;
    }
    // room for `keys` keys, at most 8 times the table per step
    uint64_t room_for(uint64_t keys) const { return std::min<uint64_t>(hist_index_slots(keys), 8 * slots); }

    // ids[at + i] = the index slot of key i (device, n keys at `stride` bytes), piece by piece,
    // before anything is linked.  grow_fn(m, done): the store's growth with `done` ids resolved;
    // m == 0 keeps the load at or below ~1/2, m != 0 makes room for a piece of m keys that did
    // not fit (GNS_E_FULL), which is then resolved again.
    using GrowFn = std::function<int(uint64_t m, uint64_t done)>;
    int resolve(const uint8_t *keys, uint32_t stride, uint64_t n, uint64_t at, hipStream_t s, const GrowFn &grow_fn);

    // every id names itself in its slot's owner word (mark); then *flag = 1 when an id is not a
    // slot or reads another's name there: two of the n rows share a slot.  The caller reads the flag.
    int own(const uint32_t *ids, uint64_t n, hipStream_t s);
    int check_unique(const uint32_t *ids, uint64_t n, uint32_t *flag, hipStream_t s);

    // A trim's rebuild beside the live table: the slots `mark` names, into a new table of `want`
    // slots (fewer allowed); dsc.remap is valid afterwards and D stays as it is until commit().
    // rollback() after any failure of the trim: the new table is freed and the claim counter the
    // rebuild restarted is set back to what the old table holds.  Both are no-ops without a
    // shrink_beside since the last of them.
    int shrink_beside(uint64_t want, hipStream_t s);
    void commit();
    void rollback();

private:
    hipError_t queue_marks(const uint32_t *const *heads, size_t nheads, hipStream_t s);  // (mark holds `slots` words)
    DictDev Dn{};  // shrink_beside's table until commit / rollback
    uint64_t slots_n = 0, live_n = 0;
    uint32_t *old_rec = nullptr;
    bool rebuilt = false, ctl_touched = false;
};

}  // namespace gns
