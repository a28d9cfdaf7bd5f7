// gns_hhplan.hpp -- the host bookkeeping of a heavy-hitter history (gns_hh_hist_*,
// gns_hhhist.hip): one table of snapshot timestamps (HistPlan, gns_histplan.hpp) shared by the
// type lanes, and per lane the log rows of snapshots 0..i.  A lane is created by the first
// append that names its type; for the snapshots before it the lane holds no rows.  Which rows
// of a lane a query as of snapshot s scans is decided here; the device holds rows only.
// No HIP here: the header compiles in a host-only driver (tests/test_heavy_history_cpu.py).
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
};

}  // namespace gns
