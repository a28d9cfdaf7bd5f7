"""gns_coldmask.cuh on the host: the expansion of a K1 block's cold-packet mask into
packet offsets, in the sub-pass windows K3s takes, against a brute-force list.  A
stand-alone program around the helper, built with ASan + UBSan (the list is written
through computed ranks)."""
import os
import shutil
import subprocess

import pytest

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gns_coldmask.cuh"

static const uint32_t W = 256, SUB = 8192, WAVES = 16;
static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }

static int check(const std::vector<uint64_t> &m, const char *what) {
    std::vector<uint32_t> want, pre(W);
    uint32_t run = 0;
    for (uint32_t i = 0; i < W; i++) {
        pre[i] = run;
        for (uint32_t l = 0; l < 64; l++)
            if ((m[i] >> l) & 1) { want.push_back(64 * i + l); run++; }
    }
    const uint32_t nsub = (run + SUB - 1) / SUB;
    for (uint32_t k = 0; k <= nsub; k++) {  // one window past the end too: nothing is written
        // exactly SUB entries: a write past the window is a heap overflow under ASan
        std::vector<uint16_t> list(SUB, (uint16_t)gns::kColdNone);
        for (uint32_t wv = 0; wv < WAVES; wv++)  // as K3s: each wave its share of the words, every lane
            for (uint32_t l = 0; l < 64; l++)
                gns::cold_expand_lane(m.data(), pre.data(), wv * (W / WAVES), (wv + 1) * (W / WAVES), l, k * SUB, SUB,
                                      list.data());
        for (uint32_t q = 0; q < SUB; q++) {
            const uint32_t rk = k * SUB + q;
            const uint32_t w = rk < run ? want[rk] : gns::kColdNone;
            if (list[q] != w) {
                std::fprintf(stderr, "%s: window %u entry %u: got %u want %u\n", what, k, q, (unsigned)list[q], w);
                return 1;
            }
        }
    }
    return 0;
}

int main() {
    std::vector<uint64_t> m(W, 0);
    if (check(m, "empty")) return 1;
    m.assign(W, ~0ull);
    if (check(m, "full")) return 1;
    m.assign(W, 0);
    m[W - 1] = 1ull << 36;
    if (check(m, "one bit in the last word")) return 1;
    m.assign(W, 0);
    m[0] = 1; m[W - 1] = 1ull << 63;
    if (check(m, "first and last bit")) return 1;
    for (int t = 0; t < 200; t++) {
        const int kind = t % 4;  // dense, half, sparse, ragged words
        for (uint32_t i = 0; i < W; i++) {
            uint64_t x = rnd();
            if (kind == 0) x |= rnd();
            if (kind == 2) x &= rnd() & rnd();
            if (kind == 3) x = (rnd() & 3) == 0 ? 0 : ((rnd() & 3) == 0 ? ~0ull : x);
            m[i] = x;
        }
        if (t % 7 == 0) for (uint32_t i = W / 2 + t; i < W; i++) m[i] = 0;  // a short last block
        if (check(m, "random")) return 1;
    }
    // exactly SUB - 1, SUB and SUB + 1 set bits
    for (uint32_t c = SUB - 1; c <= SUB + 1; c++) {
        m.assign(W, 0);
        for (uint32_t s = 0; s < c;) {
            const uint32_t p = (uint32_t)(rnd() % (64 * W));
            if (!((m[p >> 6] >> (p & 63)) & 1)) { m[p >> 6] |= 1ull << (p & 63); s++; }
        }
        if (check(m, "boundary")) return 1;
    }
    std::puts("ok");
    return 0;
}
"""


def test_cold_list_expansion_against_brute_force(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "go2netspectra_amd", "csrc")
    src, exe = tmp_path / "coldmask_driver.cpp", str(tmp_path / "coldmask_driver")
    src.write_text(DRIVER)
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, str(src), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and r.stdout.strip() == "ok", r.stderr[-3000:]
