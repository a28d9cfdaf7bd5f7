// gns_probe.hip -- self-test hook: the device float64 helpers of gns_gomath.cuh
// evaluated element by element, so a test can compare their roundings with the
// oracle's C restatements bit for bit (tests/test_gomath_gpu.py).  The S5 kernels
// of gns_ss.hip inline the same functions; in the regimes where a counter cannot
// move (b^-val subnormal or 0) an exported state does not show their results.
// Not a hot path: host arrays in, host arrays out, one launch.
#include "gns_common.hpp"
#include "gns_gomath.cuh"

namespace gns {

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void k_gomath_eval(int op, const double *x, const double *y, uint64_t n,
                                                     double *out, int32_t *out2, uint64_t seed) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double xv = x[i];
    const uint64_t xb = gm_bits(xv), yb = y ? gm_bits(y[i]) : 0ull;
    double r = 0.0;
    switch (op) {
    case GNS_GM_POW: r = go_pow_int(xv, y[i]); break;
    case GNS_GM_LDEXP: r = go_ldexp(xv, (int)(int64_t)yb); break;
    case GNS_GM_FREXP: { int e; r = go_frexp(xv, &e); out2[i] = e; break; }
    case GNS_GM_LOG: r = gm_log(xv); break;
    case GNS_GM_LOG1M: r = gm_log1m(xv); break;
    case GNS_GM_UNIFORM: r = ss_uniform(seed, xb, (uint32_t)(yb >> 32), (uint32_t)yb); break;
    case GNS_GM_HLL_SEEDS: {
        uint32_t s0, s1;
        ss_hll_seeds(seed, xb, s0, s1);
        r = gm_from((uint64_t)s1 << 32 | s0);
        break;
    }
    }
    out[i] = r;
}
#pragma clang fp contract(on)

}  // namespace gns

using namespace gns;

extern "C" int gns_gomath_eval(int op, const double *x, const double *y, uint64_t n, double *out, int32_t *out2,
                               uint64_t seed, int device) {
    const bool need_y = op == GNS_GM_POW || op == GNS_GM_LDEXP || op == GNS_GM_UNIFORM;
    if (op < GNS_GM_POW || op > GNS_GM_HLL_SEEDS || !x || !out || (need_y && !y) || (op == GNS_GM_FREXP && !out2) ||
        n > (1ull << 30)) {
        set_error("gns_gomath_eval: bad argument (op %d, n %llu)", op, (unsigned long long)n);
        return GNS_E_ARG;
    }
    if (n == 0) return GNS_OK;
    GNS_TRY(set_device(device));
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    int32_t *de = nullptr;
    auto run = [&]() -> int {
        GNS_TRY(dalloc_t(&dx, n));
        GNS_TRY(dalloc_t(&dout, n));
        GNS_HIP(hipMemcpy(dx, x, n * 8, hipMemcpyHostToDevice));
        if (need_y) {
            GNS_TRY(dalloc_t(&dy, n));
            GNS_HIP(hipMemcpy(dy, y, n * 8, hipMemcpyHostToDevice));
        }
        if (op == GNS_GM_FREXP) GNS_TRY(dalloc_t(&de, n));
        hipLaunchKernelGGL(k_gomath_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, dx, dy, n, dout, de,
                           seed);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipDeviceSynchronize());
        GNS_HIP(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
        if (op == GNS_GM_FREXP) GNS_HIP(hipMemcpy(out2, de, n * 4, hipMemcpyDeviceToHost));
        return GNS_OK;
    };
    const int rc = run();
    dfree(dx); dfree(dy); dfree(dout); dfree(de);
    return rc;
}
