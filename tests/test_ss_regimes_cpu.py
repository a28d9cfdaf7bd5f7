"""CPU: SuperSpread's rare regimes (tests/ss_regimes.py) on the two host restatements.
For every scenario the C oracle, put into the crafted state by or_ss_import, equals
pyref bit for bit after every call, and the scenario enters the regimes it declares:
a change of seeds or helpers cannot quietly turn it into an ordinary stream."""
import numpy as np
import pytest

import ss_regimes as R

NAMES = ("values", "keys", "regs", "pbits")


def same_state(got, want, what):
    """got: oracle.SuperSpread.export(); want: Census.export() (pbits as bit patterns)"""
    for name, a, b in zip(NAMES, got, want):
        if name == "pbits":
            a = a.view(np.uint64)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {name} differs"


def c_oracle(oracle, sc):
    return oracle.SuperSpread(*sc.args(), sc.seeds(), R.HLL_MASTER, R.RNG_SEED)


def test_every_regime_of_the_list_is_declared_somewhere():
    """The regimes no natural Zipf stream reaches are each a scenario's condition."""
    declared = set()
    for sc in R.scenarios():
        declared |= set(sc.need)
    assert declared >= {"lz_sat", "real_at_m1", "tempP_zero", "tempP_neg", "tempP_lt_m1", "vv_nonpos", "vv_big",
                        "foreign", "foreign_val_2048", "foreign_val_max", "decrement_at_2048", "ppp_series",
                        "ppp_subnormal", "ppp_zero", "ppp_ge1", "draw_later", "decrement",
                        "takeover_after_dec", "wait_past", "wrap"}


@pytest.mark.parametrize("name", R.names())
def test_scenario_enters_its_regimes(name):
    sc = R.by_name(name)
    _, _, counts, chain = R.reference(sc, False)
    print(name, dict(counts))
    for regime, least in sc.need.items():
        assert counts[regime] >= least, f"{name}: {regime} entered {counts[regime]} times, needs {least}"
    if sc.chain:
        assert chain[(0, 0)] == sc.chain  # one cell: the first call's chain
    if sc.mixed:  # w * d <= 64 cells: one wave walks them all
        first = [n for (cell, call), n in chain.items() if call == 0]
        print(name, "chains of the call:", sorted(first))
        assert sum(n > R.KSS_LONG_CHAIN for n in first) >= 2 and sum(n <= R.KSS_LONG_CHAIN for n in first) >= 1


@pytest.mark.parametrize("ragged", [False, True], ids=["one_call", "ragged"])
@pytest.mark.parametrize("name", R.names())
def test_c_oracle_equals_pyref(oracle, name, ragged):
    sc = R.by_name(name)
    states, _, _, _ = R.reference(sc, ragged)
    c = c_oracle(oracle, sc)
    for i, (op, want) in enumerate(zip(sc.calls(ragged), states)):
        R.apply(c, op)
        same_state(c.export(), want, f"{name} after call {i} ({op[0]})")
    p = sc.census()  # queries and the list from the final state
    p.set_state(want[0], want[1], want[2], want[3].view(np.float64), 0)
    assert c.heavy() == p.heavy()
    for f in sc.flows:
        assert c.query(bytes(f)) == p.query(bytes(f))


def test_import_sets_the_generator_position(oracle):
    sc = R.by_name("records_2pow63")
    c = c_oracle(oracle, sc)
    R.apply(c, sc.ops[0])
    assert c.packets() == 2**63 - 100
    R.apply(c, sc.ops[1])
    assert c.packets() == 2**63 - 100 + len(sc.ops[1][1])
