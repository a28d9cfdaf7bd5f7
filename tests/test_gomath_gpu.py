"""The device float64 helpers of gns_gomath.cuh, evaluated by the self-test hook
gns_gomath_eval, against the C oracle's restatements bit for bit.  The SuperSpread
state tests cannot see these roundings where a counter cannot move (b^-val subnormal
or 0: every foreign step waits past all repeats), so a build flag or a compiler that
changed one -- a fused multiply-add, a flushed subnormal, another constant -- would
pass them.  Grids: tests/gomath_grids.py (the C-against-pyref leg is test_oracle.py)."""
import numpy as np
import pytest

import gomath_grids as G

pytestmark = pytest.mark.gpu


def same_bits(got, want, x, what, y=None):
    a, b = G.bits(got), G.bits(want)
    if not np.array_equal(a, b):
        bad = np.nonzero(a != b)[0]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} differ, first at x={x[i]!r}"
                             f"{'' if y is None else f' y={y[i]!r}'}: gpu={got[i]!r} ({a[i]:#018x}) "
                             f"oracle={want[i]!r} ({b[i]:#018x})")


def test_go_pow_int(gpu, oracle):
    from go2netspectra_amd import _lib
    x, y = G.pow_grid()
    same_bits(_lib.gomath_eval(_lib.GM_POW, x, y), oracle.gomath_eval(oracle.GM_POW, x, y), x, "go_pow_int", y)


def test_go_ldexp_and_frexp(gpu, oracle):
    from go2netspectra_amd import _lib
    x, e = G.ldexp_grid()
    ey = G.as_f64(e.view(np.uint64))
    want = oracle.gomath_eval(oracle.GM_LDEXP, x, ey)
    # the grid does land on both sides of the three thresholds
    assert (want == 0).any() and np.isinf(want).any() and ((np.abs(want) > 0) & (np.abs(want) < 2.0 ** -1022)).any()
    same_bits(_lib.gomath_eval(_lib.GM_LDEXP, x, ey), want, x, "go_ldexp", e)
    fx = np.unique(np.concatenate([x, want]))
    got_f, got_e = _lib.gomath_eval(_lib.GM_FREXP, fx)
    want_f, want_e = oracle.gomath_eval(oracle.GM_FREXP, fx)
    same_bits(got_f, want_f, fx, "go_frexp fraction")
    assert np.array_equal(got_e, want_e), "go_frexp exponent"


def test_gm_log_and_log1m(gpu, oracle):
    from go2netspectra_amd import _lib
    x = G.log_grid()
    same_bits(_lib.gomath_eval(_lib.GM_LOG, x), oracle.gomath_eval(oracle.GM_LOG, x), x, "gm_log")
    p = G.log1m_grid()
    assert ((p > 0) & (p < 2.0 ** -1022)).sum() > 100 and (p < 1e-4).any() and (p >= 1e-4).any()
    same_bits(_lib.gomath_eval(_lib.GM_LOG1M, p), oracle.gomath_eval(oracle.GM_LOG1M, p), p, "gm_log1m")


def test_ss_uniform_and_hll_seeds(gpu, oracle):
    from go2netspectra_amd import _lib
    pk, rd = G.uniform_grid()
    for seed in (G.UNIFORM_SEED, 0, 2 ** 64 - 1):
        got = _lib.gomath_eval(_lib.GM_UNIFORM, G.as_f64(pk), G.as_f64(rd), seed=seed)
        want = oracle.gomath_eval(oracle.GM_UNIFORM, G.as_f64(pk), G.as_f64(rd), seed=seed)
        assert (want >= 0).all() and (want < 1).all()
        same_bits(got, want, pk, "ss_uniform", rd)
    cells = G.cells_grid()
    for master in (G.HLL_MASTER, 0, 2 ** 64 - 1):
        got = _lib.gomath_eval(_lib.GM_HLL_SEEDS, G.as_f64(cells), seed=master)
        want = oracle.gomath_eval(oracle.GM_HLL_SEEDS, G.as_f64(cells), seed=master)
        same_bits(got, want, cells, "ss_hll_seeds")


def test_bad_arguments_are_refused(gpu):
    from go2netspectra_amd import _lib
    with pytest.raises(_lib.GnsError):
        _lib.gomath_eval(99, np.ones(4))
    with pytest.raises(_lib.GnsError):
        _lib.gomath_eval(_lib.GM_POW, np.ones(4))  # no y
