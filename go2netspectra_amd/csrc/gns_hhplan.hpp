// gns_hhplan.hpp -- the host bookkeeping of a heavy-hitter history (gns_hh_hist_*,
// gns_hhhist.hip): one table of snapshot timestamps (HistPlan, gns_histplan.hpp) shared by the
// type lanes, and per lane the log rows of snapshots 0..i.  A lane is created by the first
// append that names its type; for the snapshots before it the lane holds no rows.  Which rows
// of a lane a query as of snapshot s scans is decided here, and so is what a trim expires in each
// lane and the table it leaves (trim_plan / trimmed); the device holds rows only.
// No HIP here: the header compiles in host-only drivers (tests/test_heavy_history_cpu.py,
// tests/test_heavy_history_trim_cpu.py).
// Internal: not part of the C ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "gns_histplan.hpp"

namespace gns {

enum HhHistCheck { HHH_E_TYPE = 4, HHH_E_REPEAT = 5 };  // after HistCheck's codes

constexpr uint32_t kHhTypes = 256;  // the reference's Type column is a UInt8

struct HhHistPlan {
    struct Lane {
        uint32_t type;
        uint64_t rows = 0;               // log rows of the published snapshots
        std::vector<uint64_t> end_rows;  // [snapshots] log rows of snapshots 0..i
    };
    HistPlan t;  // ts; rows / end_rows count the rows of all lanes
    std::vector<Lane> lanes;
    int lane_of[kHhTypes];

    HhHistPlan() {
        for (int &l : lane_of) l = -1;
    }
    int lane(uint32_t type) const { return type < kHhTypes ? lane_of[type] : -1; }
    // the lane of `type`, created without rows when there is none (type < kHhTypes)
    int add_lane(uint32_t type) {
        if (lane_of[type] >= 0) return lane_of[type];
        Lane l;
        l.type = type;
        l.end_rows.assign(t.ts.size(), 0);
        lanes.push_back(l);
        return lane_of[type] = (int)lanes.size() - 1;
    }
    // an append of nlists lists (types[i], ns[i] rows) under timestamp ts: HistPlan's checks --
    // the row limit holds per lane, each lane being a log of its own -- then HHH_E_TYPE for a
    // type outside 0..255 and HHH_E_REPEAT for a type named twice
    int append_check(int64_t ts, const uint32_t *types, const uint64_t *ns, uint32_t nlists) const {
        const int c = t.append_check(ts, 0);
        if (c != HIST_OK) return c;
        bool seen[kHhTypes] = {};
        for (uint32_t i = 0; i < nlists; i++) {
            if (types[i] >= kHhTypes) return HHH_E_TYPE;
            if (seen[types[i]]) return HHH_E_REPEAT;
            seen[types[i]] = true;
            const int l = lane_of[types[i]];
            if (ns[i] > kHistMax - (l >= 0 ? lanes[(size_t)l].rows : 0)) return HIST_E_ROWS;
        }
        return HIST_OK;
    }
    // the rows of lane l a query as of snapshot s scans
    uint64_t rows_as_of(int l, int64_t s) const {
        return (l < 0 || s < 0) ? 0 : lanes[(size_t)l].end_rows[(size_t)s];
    }
    // the append is complete (every type has its lane): the snapshot exists
    void publish(int64_t ts, const uint32_t *types, const uint64_t *ns, uint32_t nlists) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < nlists; i++) {
            lanes[(size_t)lane_of[types[i]]].rows += ns[i];
            total += ns[i];
        }
        for (Lane &l : lanes) l.end_rows.push_back(l.rows);
        t.publish(ts, total);
    }

    // A trim (gns_hh_hist_trim): HistPlan's plan over the shared timestamps -- c, d, fold, noop;
    // its R counts the expired rows of all lanes -- and per lane the expired prefix [0, R[l]) of
    // its log: the rows of snapshots 0..c-1, none for a lane created after snapshot c - 1.
    struct Trim {
        HistPlan::Trim t;
        std::vector<uint64_t> R;  // [lanes]
    };
    Trim trim_plan(int64_t before, bool fold) const {
        Trim x;
        x.t = t.trim_plan(before, fold);
        for (const Lane &l : lanes) x.R.push_back(x.t.c ? l.end_rows[(size_t)x.t.c - 1] : 0);
        return x;
    }
    // the plan after trim x (not a noop) kept nbase[l] rows of lane l's prefix (drop: zeros).
    // Every lane stays a lane; one that was created after the base holds zeros up to its first rows.
    HhHistPlan trimmed(const Trim &x, const std::vector<uint64_t> &nbase) const {
        HhHistPlan p;
        uint64_t total = 0;
        for (uint64_t b : nbase) total += b;
        p.t = t.trimmed(x.t, total);
        for (int i = 0; i < (int)kHhTypes; i++) p.lane_of[i] = lane_of[i];
        for (size_t l = 0; l < lanes.size(); l++) {
            const Lane &o = lanes[l];
            Lane n;
            n.type = o.type;
            if (x.t.fold) n.end_rows.push_back(nbase[l]);
            for (size_t i = (size_t)x.t.c; i < o.end_rows.size(); i++) n.end_rows.push_back(o.end_rows[i] - x.R[l] + nbase[l]);
            n.rows = o.rows - x.R[l] + nbase[l];
            p.lanes.push_back(n);
        }
        return p;
    }
};

}  // namespace gns
