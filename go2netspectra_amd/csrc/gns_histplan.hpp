// gns_histplan.hpp -- the host bookkeeping of an exact history (gns_ex_hist_*, gns_exact.hip):
// the table of snapshot timestamps, s(T) = the newest snapshot at or before a query time, the
// checks an append passes before any device call, what a trim expires and the table it leaves
// (trim_plan / trimmed), and the capacity arithmetic of the log and of the key index.  The
// device side holds rows and version words only; which snapshot a query sees is decided here.
// No HIP here: the header compiles in host-only drivers (tests/test_exact_history_cpu.py,
// tests/test_exact_history_trim_cpu.py).
// Internal: not part of the C ABI.
#pragma once
#include <cstdint>
#include <vector>

namespace gns {

// Log rows and snapshots are numbered in 32-bit version words whose all-ones value means
// "not superseded": both stay at or below 2^32 - 2.
constexpr uint64_t kHistMax = 0xFFFFFFFEull;
constexpr uint32_t kHistOpen = 0xFFFFFFFFu;

enum HistCheck { HIST_OK = 0, HIST_E_TIME = 1, HIST_E_SNAPSHOTS = 2, HIST_E_ROWS = 3 };

struct HistPlan {
    std::vector<int64_t> ts;         // strictly increasing
    std::vector<uint64_t> end_rows;  // log rows of snapshots 0..i: rows are in snapshot order
    uint64_t rows = 0;               // log rows of the published snapshots

    // s(T): the largest i with ts[i] <= T, -1 when there is none; end == nullptr: the newest
    int64_t as_of(const int64_t *end) const {
        if (!end) return (int64_t)ts.size() - 1;
        size_t lo = 0, hi = ts.size();  // ts[i] <= *end for i < lo, > *end for i >= hi
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (ts[mid] <= *end) lo = mid + 1;
            else hi = mid;
        }
        return (int64_t)lo - 1;
    }

    // an append of n rows under timestamp t: HIST_E_TIME when t does not lie after the last
    // snapshot's, HIST_E_SNAPSHOTS / HIST_E_ROWS when the log would pass kHistMax
    int append_check(int64_t t, uint64_t n) const {
        if (!ts.empty() && t <= ts.back()) return HIST_E_TIME;
        if (ts.size() >= kHistMax) return HIST_E_SNAPSHOTS;
        if (n > kHistMax - rows) return HIST_E_ROWS;
        return HIST_OK;
    }

    // the rows a query as of snapshot s scans: every row of a later snapshot lies behind them
    uint64_t rows_as_of(int64_t s) const { return s < 0 ? 0 : end_rows[(size_t)s]; }

    // A window (T0, T1] (gns_ex_hist_rollup_between): s0 = s(T0), -1 for a null start; s1 =
    // s(T1), the newest for a null end.  Rows are in snapshot order, so a row below minus_end
    // = rows_as_of(s0) was written at or before s0 and can only be a MINUS row (live at T0,
    // displaced in the window), a row from there to scan_end = rows_as_of(s1) was written in
    // the window and can only be a PLUS row (live at T1), and nothing beyond is scanned.
    // bad: both times given and T0 > T1.  empty: no snapshot at or before T1, or none in the
    // window (s0 == s1) -- nothing is scanned, whatever the row counts.
    struct Between {
        int64_t s0, s1;
        uint64_t minus_end, scan_end;
        bool bad, empty;
    };
    Between between(const int64_t *start, const int64_t *end) const {
        Between b{-1, -1, 0, 0, false, true};
        if (start && end && *start > *end) {
            b.bad = true;
            return b;
        }
        b.s1 = as_of(end);
        b.s0 = start ? as_of(start) : -1;
        if (b.s0 > b.s1) b.s0 = b.s1;  // a null end with a start after the newest snapshot
        b.empty = b.s1 < 0 || b.s0 == b.s1;
        if (!b.empty) {
            b.minus_end = rows_as_of(b.s0);
            b.scan_end = rows_as_of(b.s1);
        }
        return b;
    }

    // the append is complete: snapshot ts.size() exists
    void publish(int64_t t, uint64_t n) {
        ts.push_back(t);
        rows += n;
        end_rows.push_back(rows);
    }

    // A trim (gns_ex_hist_trim): the c snapshots with ts < before expire, a prefix of the log
    // of R rows.  Drop removes them; fold keeps of them the rows live as of snapshot c - 1 as
    // the new snapshot 0 under ts[c - 1].  d: what every version word of a remaining row
    // loses (a word below d becomes 0: the row then belongs to the base).  A plan with c == 0,
    // or with c == 1 under fold (the base is snapshot 0 itself), moves nothing.
    struct Trim {
        uint64_t c, R;
        uint32_t d;
        bool fold, noop;
    };
    Trim trim_plan(int64_t before, bool fold) const {
        size_t lo = 0, hi = ts.size();  // ts[i] < before for i < lo, >= before for i >= hi
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (ts[mid] < before) lo = mid + 1;
            else hi = mid;
        }
        Trim t;
        t.c = lo;
        t.R = lo ? end_rows[lo - 1] : 0;
        t.fold = fold;
        t.d = (uint32_t)(fold && lo ? lo - 1 : lo);
        t.noop = lo == 0 || (fold && lo == 1);
        return t;
    }
    // the plan after trim t (not a noop) kept nbase rows of the prefix (drop: 0)
    HistPlan trimmed(const Trim &t, uint64_t nbase) const {
        HistPlan p;
        if (t.fold) {
            p.ts.push_back(ts[t.c - 1]);
            p.end_rows.push_back(nbase);
        }
        for (size_t i = t.c; i < ts.size(); i++) {
            p.ts.push_back(ts[i]);
            p.end_rows.push_back(end_rows[i] - t.R + nbase);
        }
        p.rows = rows - t.R + nbase;
        return p;
    }
};

// Row capacity of a log of `cap` rows that is to hold `need`: unchanged when it fits, else
// doubled (from at least 1) until it does, never beyond kHistMax.  need <= kHistMax.
inline uint64_t hist_row_capacity(uint64_t cap, uint64_t need) {
    if (need <= cap) return cap;
    uint64_t c = cap ? cap : 1;
    while (c < need) c = c > kHistMax / 2 ? kHistMax : c * 2;
    return c;
}

// Slots of a key index that holds `flows` distinct keys at a load of at most 1/2: a power of
// two, at least 64.
inline uint64_t hist_index_slots(uint64_t flows) {
    uint64_t s = 64;
    while (s < 2 * flows) s <<= 1;
    return s;
}

// two layouts name the same key bytes (src: the tuple byte of every key byte, make_plan's numbering)
inline bool hist_same_layout(const uint8_t *a, uint32_t ka, const uint8_t *b, uint32_t kb) {
    if (ka != kb) return false;
    for (uint32_t i = 0; i < ka; i++)
        if (a[i] != b[i]) return false;
    return true;
}

}  // namespace gns
