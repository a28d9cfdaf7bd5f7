// gns_exsrc.hpp -- what another engine may see of an exact aggregator's resident
// table (gns_exact.hip keeps struct gns_ex private): a read-only reference for
// kernels that project its flows elsewhere (gns_spread_rollup in gns_spread.hip).
// Also the device half of the projection both roll-ups share (gns_ex_rollup[_prefix],
// gns_spread_rollup[_prefix]; the plan is gns_rollplan.hpp's): a lane's LDS key column, the
// address-class test, the EncodeFlow rewrite, the gathered word and the stored row; and the
// range check of a gns_prefix.
// Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gns_common.hpp"
#include "gns_keys.cuh"
#include "gns_rollplan.hpp"

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

// ::ffff:a.b.c.d -> a.b.c.d + 12 zero bytes in the 16 key bytes at offset o (uniform) of the
// lane's column; every other value stays
__device__ __forceinline__ void spr_encode_ip(uint32_t (*s_k)[256], uint32_t tid, uint32_t o) {
    if ((o & 3u) == 0u) {
        const uint32_t w = o >> 2;
        if (s_k[w][tid] == 0u && s_k[w + 1][tid] == 0u && s_k[w + 2][tid] == 0xFFFF0000u) {
            s_k[w][tid] = s_k[w + 3][tid];
            s_k[w + 1][tid] = 0u; s_k[w + 2][tid] = 0u; s_k[w + 3][tid] = 0u;
        }
    } else {
        uint8_t *col = reinterpret_cast<uint8_t *>(&s_k[0][tid]);  // key byte b: word b / 4 of the column, byte b % 4
        auto at = [&](uint32_t b) -> uint8_t & { return col[(size_t)(b >> 2) * (256 * 4) + (b & 3u)]; };
        uint32_t z = 0;
#pragma unroll
        for (uint32_t k = 0; k < 10; k++) z |= at(o + k);
        if (z == 0u && at(o + 10) == 0xFFu && at(o + 11) == 0xFFu) {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) at(o + k) = at(o + 12 + k);
#pragma unroll
            for (uint32_t k = 4; k < 16; k++) at(o + k) = 0;
        }
    }
}

// The key words of record r (load_record's: r[0] is the tag) into the lane's own column, to be
// read back byte by byte through the plan.  No other lane touches the column, so no barrier is
// needed and a wave without flows may leave.
__device__ __forceinline__ void proj_fill_column(uint32_t (*s_k)[256], uint32_t tid, const uint32_t *r) {
#pragma unroll
    for (int i = 0; i < GNS_KWMAX; i++) s_k[i][tid] = r[1 + i];
}

// Word i of a K-byte row gathered from the lane's column.  t: the row's gather index g, one
// byte per row byte.  PX: masked as well -- t is a whole RollRow (g, fld, m4, m6 at 40 bytes
// each) and v4 has bit f set when IP field f of this flow is IPv4:
// byte j = column byte g[j] & (v4[fld[j]] ? m4[j] : m6[j]), branch-free, any bit length.
template <bool PX>
__device__ __forceinline__ uint32_t proj_word(const uint32_t (*s_k)[256], uint32_t tid, const uint8_t *t, uint32_t v4,
                                              uint32_t K, int i) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int j = 4 * i + b;
        if ((uint32_t)j < K) {
            const uint32_t g = t[j];
            uint32_t mk = 0xFFu;
            if constexpr (PX) mk = (v4 >> t[40 + j] & 1u) ? t[80 + j] : t[120 + j];
            v |= ((s_k[g >> 2][tid] >> (8u * (g & 3u))) & mk) << (8 * b);
        }
    }
    return v;
}

// A K-byte row of proj_word's words to `row`.  WORDS: K is a multiple of 4 and the row
// word-aligned; otherwise byte stores, so a row may start and end inside a word.
template <bool PX, bool WORDS>
__device__ __forceinline__ void proj_store_row(const uint32_t (*s_k)[256], uint32_t tid, const uint8_t *t, uint32_t v4,
                                               uint32_t K, uint8_t *row) {
#pragma unroll
    for (int i = 0; i < GNS_KWMAX; i++) {
        if (4u * i >= K) break;  // uniform
        uint32_t v = 0;
        if constexpr (PX) {
            v = proj_word<true>(s_k, tid, t, v4, K, i);
        } else {
            // proj_word<false>, written out: through the call the compiler leaves this loop over the
            // words rolled in k_spr_project<false, true> (2764 instructions against 6745); written
            // out, that kernel is instruction for instruction what it was
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int j = 4 * i + b;
                if ((uint32_t)j < K) {
                    const uint32_t g = t[j];
                    v |= ((s_k[g >> 2][tid] >> (8u * (g & 3u))) & 0xFFu) << (8 * b);
                }
            }
        }
        if constexpr (WORDS) {
            reinterpret_cast<uint32_t *>(row)[i] = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if ((uint32_t)(4 * i + b) < K) row[4 * i + b] = (uint8_t)(v >> (8 * b));
        }
    }
}

}  // namespace gns
