// gns_pinchunk.hpp -- the host arithmetic of PinnedOut::copy_out (gns_common.hpp):
// device bytes reach pageable host memory piece by piece through pinned chunks.
// Nothing here calls the runtime, so tests/pin_chunks_check.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace gns {

// sw != 0: the source is rows of sw bytes of which the first dw <= sw go out (key words
// -> key bytes).  A piece is the part of a chunk that holds whole rows.
inline size_t pin_piece(size_t chunk, size_t sw) { return sw ? chunk - chunk % sw : chunk; }
inline size_t pin_pieces(size_t bytes, size_t piece) { return (bytes + piece - 1) / piece; }
// source offset and length of piece i
inline size_t pin_off(size_t i, size_t piece) { return i * piece; }
inline size_t pin_len(size_t i, size_t piece, size_t bytes) { return std::min(piece, bytes - i * piece); }
// piece i of `bytes` source bytes has landed at p: its bytes, or its rows narrowed, to their place in dst
inline void pin_land(uint8_t *dst, const uint8_t *p, size_t i, size_t piece, size_t bytes, size_t sw, size_t dw) {
    const size_t off = pin_off(i, piece), m = pin_len(i, piece, bytes);
    if (!sw || sw == dw) {
        memcpy(dst + off, p, m);
    } else {
        uint8_t *o = dst + off / sw * dw;
        for (size_t r = 0; r < m / sw; r++) memcpy(o + r * dw, p + r * sw, dw);
    }
}

}  // namespace gns
