// gns_exsrc.hpp -- what another engine may see of an exact aggregator's resident
// table (gns_exact.hip keeps struct gns_ex private): a read-only reference for
// kernels that project its flows elsewhere (gns_spread_rollup in gns_spread.hip).
// Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gns_keys.cuh"

struct gns_ex;

namespace gns {

// Valid until the next ingest-side call on the handle (a growth moves the table).
struct ExTableRef {
    int device;
    hipStream_t stream;               // the handle's stream: record an event on it before reading the table
    KeyPlanN kp;                      // key layout: kp.src[j] = tuple byte of key byte j
    DictDev D;                        // records {tag, key words in To16 form}
    uint64_t slots;
    const unsigned long long *pkts;   // [slots] a slot holds a flow iff its tag and pkts are nonzero (k_ex_list)
    const unsigned long long *first;  // [slots] stream position of the flow's first packet or merged row
    uint64_t pos;                     // the next stream position: the cursor gns_ex_view_refresh returns
};

void ex_table_ref(const gns_ex *ex, ExTableRef *out);

}  // namespace gns
