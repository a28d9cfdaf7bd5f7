"""gns_pinchunk.hpp on the host: the piece arithmetic of PinnedOut::copy_out (a view's
export through two pinned chunks, key-word rows narrowed to key bytes) against a naive
per-row copy.  A stand-alone program around the header, built with ASan + UBSan: the two
chunks and the destination are heap blocks of exactly their size, so a piece that
overruns a chunk or a row that lands outside the destination is reported."""
import os
import shutil
import subprocess

import pytest

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gns_pinchunk.hpp"

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }

// PinnedOut::copy_out with memcpy for the device copy and `chunk` for kPinChunk
static int check(size_t chunk, size_t bytes, size_t sw, size_t dw) {
    std::vector<uint8_t> src(bytes);
    for (auto &b : src) b = (uint8_t)rnd();
    // (rows as wide as the source are a plain copy, a trailing part of a row included)
    const bool narrow = sw && dw != sw;
    const size_t rows = narrow ? bytes / sw : 0, out_bytes = narrow ? rows * dw : bytes;
    std::vector<uint8_t> want(out_bytes);
    if (narrow) {
        for (size_t r = 0; r < rows; r++)
            for (size_t i = 0; i < dw; i++) want[r * dw + i] = src[r * sw + i];
    } else {
        want = src;
    }
    uint8_t *half[2] = {(uint8_t *)malloc(chunk), (uint8_t *)malloc(chunk)};
    uint8_t *dst = (uint8_t *)malloc(out_bytes ? out_bytes : 1);
    const size_t piece = gns::pin_piece(chunk, sw), n = gns::pin_pieces(bytes, piece);
    int bad = 0;
    if (piece == 0 || piece > chunk || (sw && piece % sw)) bad = 1;
    size_t covered = 0;
    for (size_t j = 0; j <= n && !bad; j++) {
        if (j < n) {
            const size_t off = gns::pin_off(j, piece), len = gns::pin_len(j, piece, bytes);
            if (off != covered || len == 0 || len > chunk) { bad = 2; break; }
            memcpy(half[j & 1], src.data() + off, len);  // ASan: inside the chunk and the source
            covered += len;
        }
        if (j > 0) gns::pin_land(dst, half[(j - 1) & 1], j - 1, piece, bytes, sw, dw);
    }
    if (!bad && covered != bytes) bad = 3;
    if (!bad && out_bytes && memcmp(dst, want.data(), out_bytes)) bad = 4;
    free(half[0]); free(half[1]); free(dst);
    if (bad) std::fprintf(stderr, "chunk %zu bytes %zu sw %zu dw %zu: failure %d\n", chunk, bytes, sw, dw, bad);
    return bad;
}

int main() {
    const size_t sws[4] = {0, 4, 12, 40};
    const size_t dws[4][4] = {{0, 0, 0, 0}, {4, 3, 1, 2}, {12, 9, 5, 8}, {40, 37, 1, 22}};
    for (size_t chunk : {500, 480, 256}) {  // 500 is a multiple of 4 only, 480 of all three, 256 of 4
        for (int a = 0; a < 4; a++) {
            const size_t sw = sws[a];
            const size_t sizes[6] = {0, sw, chunk - sw, chunk, chunk + sw, 3 * chunk + sw};
            for (int b = 0; b < (sw ? 4 : 1); b++)
                for (size_t bytes : sizes) {
                    if (check(chunk, bytes, sw, dws[a][b])) return 1;
                    // whole rows (what the views pass) next to the size
                    if (sw && check(chunk, bytes / sw * sw, sw, dws[a][b])) return 1;
                }
        }
    }
    if (check(500, 1, 0, 0) || check(500, 499, 0, 0) || check(500, 501, 0, 0) || check(500, 2000, 0, 0)) return 1;
    std::puts("ok");
    return 0;
}
"""


def test_pinned_pieces_against_per_row_copy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "go2netspectra_amd", "csrc")
    src, exe = tmp_path / "pinchunk_driver.cpp", str(tmp_path / "pinchunk_driver")
    src.write_text(DRIVER)
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, str(src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and r.stdout.strip() == "ok", r.stderr[-3000:]
