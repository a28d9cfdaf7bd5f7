"""SuperSpread's sequential step (S5: k_ss_walk_pbits, k_ss_sample, k_ss_walk_mv) in the
regimes no natural Zipf stream enters -- tests/ss_regimes.py lists them and
test_ss_regimes_cpu.py proves that every scenario enters the ones it declares.

After every call the device equals the C oracle: values, keys and registers equal,
pbits as uint64 bit patterns, the heavy-hitter list at threshold 1, the query of every
flow, and the number of HLL encodes (the census's count).  Every scenario runs twice:
each insert as one call, which must be one device batch, so that a cell's whole chain is
walked at once; and the same packets in ragged calls of 1, 47, 48, 49, 63, 64, 65, 255,
257, ... packets.  The chain_L scenarios cut a single-cell stream so that the first
call's chain is exactly L encodes, for L on both sides of kSsLongChain (48), of the
64-lane window and of the four windows in flight (256); the crafted `val` states sit on
both sides of kSsMvTab (2048).

pbits stays finite throughout: NaN or inf cannot arise from a stream, and NaN payload
propagation differs between x86 and the GPU, so such imports are out of scope."""
import numpy as np
import pytest

import ss_regimes as R
from helpers import assert_same_list

pytestmark = pytest.mark.gpu

NAMES = ("values", "keys", "regs", "pbits")


def assert_same_state(ss, orc, what):
    for name, a, b in zip(NAMES, ss.export_state(), orc.export()):
        if name == "pbits":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0] if a.ndim == 1 else np.nonzero((a != b).any(axis=1))[0]
            raise AssertionError(f"{what}: {name} differs in {len(bad)} cells, first {bad[:5]}: "
                                 f"gpu={a[bad[:3]]} oracle={b[bad[:3]]}")


@pytest.mark.parametrize("ragged", [False, True], ids=["one_call", "ragged"])
@pytest.mark.parametrize("name", R.names())
def test_device_equals_oracle_after_every_call(gpu, oracle, name, ragged):
    from go2netspectra_amd import SuperSpread
    sc = R.by_name(name)
    _, encodes, _, _ = R.reference(sc, ragged)
    w, d, thr, m, size, base, b, kf, ke = sc.args()
    ss = SuperSpread(w, d, thr, m, size, base, b, flow_bytes=kf, elem_bytes=ke, seeds=sc.seeds(),
                     hll_master=R.HLL_MASTER, rng_seed=R.RNG_SEED)
    orc = oracle.SuperSpread(*sc.args(), sc.seeds(), R.HLL_MASTER, R.RNG_SEED)
    inserts = 0
    for i, (op, enc) in enumerate(zip(sc.calls(ragged), encodes)):
        R.apply(ss, op)
        R.apply(orc, op)
        inserts += op[0] == "insert"
        what = f"{name} after call {i} ({op[0]})"
        assert_same_state(ss, orc, what)
        got_hh = [(h.Flow, h.Count) for h in ss.heavy_hitters().Count]
        assert_same_list(got_hh, orc.heavy(), what + ": heavy hitters")
        want_q = np.array([orc.query(bytes(f)) for f in sc.flows], np.uint64)
        assert np.array_equal(ss.query_many(sc.flows), want_q), what + ": queries"
        c = ss.counters()
        assert c["encodes"] == enc, what + ": encodes"
        assert c["batches"] == inserts, what + ": every call is one device batch"
    ss.close()
