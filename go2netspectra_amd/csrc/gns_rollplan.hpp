// gns_rollplan.hpp -- the plan of a roll-up, on the host: which byte of the source's key
// every byte of a destination row comes from, and the prefix mask it is stored under.  One
// definition for gns_ex_rollup[_prefix] (gns_exact.hip) and gns_spread_rollup[_prefix]
// (gns_spread.hip, once per row: flow, element); exact.py restates it (rollup_plan,
// prefix_plan, spread_rollup_plan) and tests/test_rollplan_cpu.py holds the two together.
// No HIP here: the header compiles in a host-only driver.
// Internal: not part of the C ABI.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/gns_sketch.h"

namespace gns {

// the mask byte of byte b of a value whose leading `bits` bits are kept
inline uint8_t px_prefix_byte(uint32_t bits, uint32_t b) {
    if (8 * b + 8 <= bits) return 0xFF;
    if (8 * b >= bits) return 0;
    return (uint8_t)(0xFF00u >> (bits - 8 * b));
}

// the key field tuple byte t belongs to (make_plan's numbering)
inline const char *tuple_field_name(uint32_t t) {
    return t < 16 ? "SrcIP" : t < 32 ? "DstIP" : t < 34 ? "SrcPort" : t < 36 ? "DstPort" : "Protocol";
}

// Byte gather between two layouts (src[i], dst[j]: the tuple byte of key byte i, j): g[j] = the
// first place the source's key holds byte j of the destination row.  Returns -1, or the first
// j whose field is not part of the source.
inline int roll_gather(const uint8_t *src, uint32_t K, const uint8_t *dst, uint32_t n, uint8_t *g) {
    for (uint32_t j = 0; j < n; j++) {
        uint32_t i = 0;
        while (i < K && src[i] != dst[j]) i++;
        if (i == K) return (int)j;
        g[j] = (uint8_t)i;
    }
    return -1;
}

// The tables of one destination row of <= 40 bytes, laid out as the projection kernels read them
// from LDS.  Per row byte j: the gather index g, the IP field the byte belongs to (0 SrcIP,
// 1 DstIP, 2 none) and two mask bytes: m4 applies when the field's value is IPv4, m6 when it is
// anything else; bytes outside IP fields carry 0xff in both.
struct RollRow {
    uint8_t g[40], fld[40], m4[40], m6[40];
};

// roll_gather into row->g with the row's field and mask tables.  px == nullptr keeps every bit
// (all masks 0xff); a prefix for a field the row lacks leaves no trace.  m4 counts the IPv4
// prefix where the address sits when the mask is applied: bytes 12..15 of the To16 form
// (::ffff:a.b.c.d, bytes 0..11 kept), or with `encodeflow` bytes 0..3 of the EncodeFlow form
// (a.b.c.d + 12 zero bytes).  ipoff[f] becomes the byte offset of IP field f in the source's
// key when the row reads it (fields are gathered whole: the field starts where its byte 0
// does); other entries are left alone, so the caller presets 0xFF (not read) once and may
// build several rows over one ipoff.
inline int roll_tables(const uint8_t *src, uint32_t K, const uint8_t *dst, uint32_t n, const gns_prefix *px,
                       bool encodeflow, RollRow *row, uint8_t ipoff[2]) {
    memset(row, 0, sizeof(*row));
    const int miss = roll_gather(src, K, dst, n, row->g);
    if (miss >= 0) return miss;
    const uint32_t v4[2] = {px ? px->src_v4 : 32u, px ? px->dst_v4 : 32u};
    const uint32_t v6[2] = {px ? px->src_v6 : 128u, px ? px->dst_v6 : 128u};
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t t = dst[j];
        if (t >= 32) { row->fld[j] = 2; row->m4[j] = row->m6[j] = 0xFF; continue; }
        const uint32_t f = t >> 4, b = t & 15u, b4 = encodeflow ? b : b - 12;  // b4 >= 4: outside the address
        row->fld[j] = (uint8_t)f;
        row->m4[j] = b4 < 4 ? px_prefix_byte(v4[f], b4) : 0xFF;
        row->m6[j] = px_prefix_byte(v6[f], b);
        if (b == 0) ipoff[f] = row->g[j];
    }
    return -1;
}

}  // namespace gns
