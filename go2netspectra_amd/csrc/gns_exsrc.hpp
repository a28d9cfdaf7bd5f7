// gns_exsrc.hpp -- what another engine may see of an exact aggregator's resident
// table (gns_exact.hip keeps struct gns_ex private): a read-only reference for
// kernels that project its flows elsewhere (gns_spread_rollup in gns_spread.hip).
// Also the one definition of the prefix mask both roll-ups apply (gns_ex_rollup_prefix,
// gns_spread_rollup_prefix): the address-class test, the mask byte, the range check and the
// masked byte gather.
// Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gns_common.hpp"
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

// --- the prefix mask -----------------------------------------------------------
// the mask byte of byte b of a value whose leading `bits` bits are kept
inline uint8_t px_prefix_byte(uint32_t bits, uint32_t b) {
    if (8 * b + 8 <= bits) return 0xFF;
    if (8 * b >= bits) return 0;
    return (uint8_t)(0xFF00u >> (bits - 8 * b));
}

// GNS_E_ARG for a null gns_prefix or one outside {0..32, 0..128, 0..32, 0..128}
inline int px_check_prefix(const gns_prefix *px, const char *what) {
    if (!px) { set_error("null argument"); return GNS_E_ARG; }
    if (px->src_v4 > 32 || px->dst_v4 > 32 || px->src_v6 > 128 || px->dst_v6 > 128) {
        set_error("%s: prefix {%u,%u,%u,%u} outside {0..32, 0..128, 0..32, 0..128}", what, px->src_v4, px->src_v6,
                  px->dst_v4, px->dst_v6);
        return GNS_E_ARG;
    }
    return GNS_OK;
}

// The address class: the 16 key bytes at offset o (uniform) of the lane's column of s_k (key
// word w of lane tid at s_k[w][tid]) hold ::ffff:a.b.c.d -- bytes 0..9 zero, bytes 10, 11 ff ff.
__device__ __forceinline__ bool px_is_v4(const uint32_t (*s_k)[256], uint32_t tid, uint32_t o) {
    if ((o & 3u) == 0u) {
        const uint32_t w = o >> 2;
        return s_k[w][tid] == 0u && s_k[w + 1][tid] == 0u && s_k[w + 2][tid] == 0xFFFF0000u;
    }
    auto at = [&](uint32_t b) -> uint32_t { return (s_k[b >> 2][tid] >> (8u * (b & 3u))) & 0xFFu; };
    uint32_t z = 0;
#pragma unroll
    for (uint32_t k = 0; k < 10; k++) z |= at(o + k);
    return z == 0u && at(o + 10) == 0xFFu && at(o + 11) == 0xFFu;
}

// Word i of a K-byte row gathered from the lane's column and masked.  t: the row's tables, 40
// bytes each -- gather index g, IP field fld (0 SrcIP, 1 DstIP, 2 none), m4, m6; v4: bit f set
// when IP field f of this flow is IPv4.  Byte j = column byte g[j] & (v4[fld[j]] ? m4[j] : m6[j]).
__device__ __forceinline__ uint32_t px_masked_word(const uint32_t (*s_k)[256], uint32_t tid, const uint8_t *t, uint32_t v4,
                                                   uint32_t K, int i) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int j = 4 * i + b;
        if ((uint32_t)j < K) {
            const uint32_t g = t[j], f = t[40 + j];
            const uint32_t mk = (v4 >> f & 1u) ? t[80 + j] : t[120 + j];
            v |= ((s_k[g >> 2][tid] >> (8u * (g & 3u))) & mk) << (8 * b);
        }
    }
    return v;
}

}  // namespace gns
