"""Input grids for the Go-math helpers (go_pow_int, go_ldexp, go_frexp, gm_log,
gm_log1m, ss_uniform, ss_hll_seeds), shared by the C-against-pyref leg
(test_oracle.py) and the device-against-C leg (test_gomath_gpu.py).  Each grid is
built once and never modified."""
import functools

import numpy as np

POW_B = (1.08, 1.2, 2.0, 1e6, 0.9, 0.5, 0.7, 1.0)   # SuperSpread's b: b^-val, val up to 12000
POW_BASE = (0.5, 0.7, 0.999, 1e-3)                  # SuperSpread's base: base^k, k a register value
UNIFORM_SEED = 0x0DDBA11CAFEF00D5
HLL_MASTER = 0x0123456789ABCDEF


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def as_f64(u):
    """integers as the bit patterns of float64 (how the eval calls take them)"""
    return np.ascontiguousarray(u, np.uint64).view(np.float64)


@functools.lru_cache(None)
def pow_grid():
    """(x, y): b^(+-v) for v in [0, 12000] and every b, then base^k for k in [0, 255]"""
    v = np.arange(0, 12001, dtype=np.float64)
    xs, ys = [], []
    for b in POW_B:
        xs += [np.full(v.size, b), np.full(v.size, b)]
        ys += [v, -v]
    k = np.arange(0, 256, dtype=np.float64)
    for base in POW_BASE:
        xs.append(np.full(k.size, base))
        ys.append(k)
    return np.concatenate(xs), np.concatenate(ys)


@functools.lru_cache(None)
def ldexp_grid():
    """(frac, e int64): normal, subnormal, zero and inf fractions; for each, exponents that
    put the result's exponent on both sides of -1075 (zero), -1022 (subnormal) and 1023 (inf)"""
    rng = np.random.default_rng(11)
    fr = [1.0, -1.0, 1.5, 0.75, -1.25, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 2.0 ** -1022, 2.0 ** 1023,
          1.7976931348623157e308, 2.2250738585072014e-308, 5e-324, -5e-324, 2.0 ** -1060, 3 * 2.0 ** -1074,
          2.225073858507201e-308, 0.0, -0.0, np.inf, -np.inf]
    fr += list(rng.random(20) + 0.5)                                   # normal, random mantissas
    fr += list((rng.random(10) + 0.5) * 2.0 ** -1040)                  # subnormal, random mantissas
    fr += list(as_f64(rng.integers(1, 2 ** 52, 10, dtype=np.uint64)))  # subnormal bit patterns
    fr = np.array(fr, np.float64)
    targets = np.concatenate([np.arange(-1082, -1066), np.arange(-1028, -1016), np.arange(1018, 1030),
                              [0, 1, -1, 52, -52, 53, -53, 2000, -2000, 5000, -5000, 100000, -100000]])
    xs, es = [], []
    for f in fr:
        ef = int(np.frexp(f)[1]) if np.isfinite(f) and f != 0 else 0
        e = targets - ef  # result exponent = target
        xs.append(np.full(e.size, f))
        es.append(e)
    return np.concatenate(xs), np.concatenate(es).astype(np.int64)


@functools.lru_cache(None)
def log_grid():
    """1.0, 1 - 2^-53, sqrt(1/2) and both neighbours, every power of two down to the smallest
    subnormal, 10^5 random points of (0, 1]"""
    rng = np.random.default_rng(12)
    r = np.float64(0.70710678118654752440)
    x = [1.0, 1.0 - 2.0 ** -53, r, np.nextafter(r, 0.0), np.nextafter(r, 1.0), 0.5, np.nextafter(0.5, 0.0),
         np.nextafter(0.5, 1.0)]
    x += [2.0 ** -k for k in range(0, 1075)]
    return np.concatenate([np.array(x, np.float64), 1.0 - rng.random(100_000)])


@functools.lru_cache(None)
def log1m_grid():
    """both neighbours of 1e-4, subnormal p, 1 - 2^-53, and every b^-v of pow_grid in (0, 1)"""
    from oracle import oracle
    t = np.float64(1e-4)
    p = [t, np.nextafter(t, 0.0), np.nextafter(t, 1.0), 5e-324, 2.0 ** -1060, 1e-310, 2.2250738585072014e-308,
         np.nextafter(2.2250738585072014e-308, 0.0), 1.0 - 2.0 ** -53, 0.5, 1e-17, 1e-300]
    x, y = pow_grid()
    pw = oracle.gomath_eval(oracle.GM_POW, x, y)
    return np.concatenate([np.array(p, np.float64), pw[(pw > 0) & (pw < 1)]])


@functools.lru_cache(None)
def uniform_grid():
    """(pkt u64, row << 32 | draw u64): packets around 2^27, 2^32 and 2^63, rows 0-7, draws 0-40"""
    pkts = [0, 1, 2 ** 64 - 1]
    for c in (2 ** 27, 2 ** 32, 2 ** 63):
        pkts += [c - 2, c - 1, c, c + 1, c + 2]
    pk, rd = [], []
    for p in pkts:
        for row in range(8):
            for draw in range(41):
                pk.append(p)
                rd.append(row << 32 | draw)
    return np.array(pk, np.uint64), np.array(rd, np.uint64)


@functools.lru_cache(None)
def cells_grid():
    rng = np.random.default_rng(13)
    return np.concatenate([np.arange(0, 2048, dtype=np.uint64), rng.integers(0, 2 ** 63, 500, dtype=np.uint64) * 2 + 1,
                           np.array([2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1], np.uint64)])
