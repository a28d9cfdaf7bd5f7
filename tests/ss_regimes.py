"""SuperSpread's sequential step in its rare regimes: a census of the branches a
stream enters, and the scenarios that enter them (shared by test_ss_regimes_cpu.py
and test_ss_regimes_gpu.py).

The census is oracle/pyref.py's SuperSpreadSeq with its `_note` hook overridden: the
class calls the hook in every branch, the census counts the calls, so no arithmetic
is restated here.  Regime names:

  encode              a real HLL update (lz above the register)
  lz_sat              ... whose lz is 2^size - 1 (super_spread.go:107 adds nothing)
  real_at_m1          ... whose tempP is exactly -1.0: Go's :196 test drops it
  tempP_zero / tempP_neg / tempP_lt_m1
                      inv = inf, pCU = NaN, vv = MinInt64 / vv < 0 / ceil = -0.0, pCU = +inf, vv = 0
  vv_nonpos / vv_big  sampled with vv <= 0 / vv >= 2^31
  foreign             an MV step on a counter another flow owns
  foreign_val_2048    ... with val >= kSsMvTab (no LDS table on the device)
  foreign_val_max     ... with val = 2^32 - 1
  decrement_at_2048   a decrement of a counter at exactly kSsMvTab
  ppp_series          b^-val < 1e-4 (log1m's series branch)
  ppp_subnormal / ppp_zero / ppp_ge1
  draw_later          second and later uniform of one encode
  decrement / takeover_after_dec / wait_past
  wrap                the owner's add wraps the u32 counter

`chain[(cell, call)]` counts the encodes of a cell inside one insert call: the chain
the device walks.  The device constants the numbers below straddle (gns_ss.hip):
kSsLongChain = 48 (lane per cell up to 48 encodes, the whole wave above), the
64-lane window of the wave walk, its four windows in flight (256 encodes) and
kSsMvTab = 2048 (b^-val from LDS below, computed above).  If they move, CHAIN_L,
RAGGED and the crafted `val` lists move with them.
"""
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from oracle import pyref

HLL_MASTER, RNG_SEED = 0x0123456789ABCDEF, 0x0DDBA11CAFEF00D5
KF = KE = 4
KSS_MV_TAB = 2048     # gns_ss.hip kSsMvTab: b^-val comes from an LDS table below it
KSS_LONG_CHAIN = 48   # gns_ss.hip kSsLongChain: chains above it are walked by the whole wave
# chain lengths around kSsLongChain, the 64-lane window and the 4 x 64 prefetch depth
CHAIN_L = [1, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320]
# ragged call sizes, cycled over a scenario's packets
RAGGED = [1, 47, 48, 49, 63, 64, 65, 255, 257, 127, 128, 129, 256, 320, 511, 513]


class Census(pyref.SuperSpreadSeq):
    def __init__(self, *a):
        super().__init__(*a)
        self.counts = Counter()
        self.chain = Counter()
        self.call = 0

    def _note(self, what, cell=-1, val=-1):
        self.counts[what] += 1
        if what == "encode":
            self.chain[(cell, self.call)] += 1
        elif what == "foreign":
            if val >= KSS_MV_TAB:
                self.counts["foreign_val_2048"] += 1
            if val == 0xFFFFFFFF:
                self.counts["foreign_val_max"] += 1
        elif what in ("decrement", "ppp_ge1") and val == KSS_MV_TAB:
            self.counts["decrement_at_2048"] += 1

    def insert_call(self, fl, el):
        """One insert call: its encodes form the cells' chains of this call."""
        for f, e in zip(fl, el):
            self.insert(bytes(f), bytes(e))
        self.call += 1

    def export(self):
        """(values u32, keys [n, KF] u8, regs [n, m] u8, pbits bit patterns u64)"""
        keys = np.frombuffer(b"".join(self.keys), np.uint8).reshape(len(self.keys), self.kf)
        return (np.array(self.values, np.uint32), keys, np.array(self.regs, np.uint8),
                np.array(self.pbits, np.float64).view(np.uint64))


@dataclass
class Scenario:
    name: str
    w: int
    d: int
    m: int
    size: int
    base: float
    b: float
    # ("insert", flows, elems) | ("reset",) | ("import", values, keys, regs, pbits, records)
    ops: list = field(default_factory=list)
    need: dict = field(default_factory=dict)  # regime -> the least count the reference must reach
    flows: np.ndarray = None                  # every flow of the stream (queries)
    chain: int = 0                            # > 0: the first insert's longest chain is exactly this
    mixed: bool = False                       # the first insert holds long chains and short ones together

    def seeds(self):
        return np.random.default_rng(self.w * 131 + self.d).integers(0, 2**32, self.d, dtype=np.uint64).astype(
            np.uint32)

    def args(self, thr=1):
        return (self.w, self.d, thr, self.m, self.size, self.base, self.b, KF, KE)

    def census(self):
        return Census(*self.args(), self.seeds().tolist(), HLL_MASTER, RNG_SEED)

    def calls(self, ragged):
        """The ops with every insert kept whole (one device batch) or cut into RAGGED calls."""
        k = 0
        for op in self.ops:
            if op[0] != "insert" or not ragged:
                yield op
                continue
            fl, el = op[1], op[2]
            off = 0
            while off < len(fl):
                n = RAGGED[k % len(RAGGED)]
                k += 1
                yield ("insert", fl[off:off + n], el[off:off + n])
                off += n


def apply(side, op):
    """One op on a Census, an oracle.SuperSpread or a device SuperSpread."""
    if op[0] == "insert":
        if isinstance(side, Census):
            side.insert_call(op[1], op[2])
        elif hasattr(side, "insert_keys"):
            side.insert_keys(op[1], op[2])
            side.flush()
        else:
            side.insert(op[1], op[2])
    elif op[0] == "reset":
        side.reset()
    else:
        _, values, keys, regs, pbits, records = op
        if isinstance(side, Census):
            side.set_state(values, keys, regs, pbits, records)
        else:
            side.import_state(values, keys, regs, pbits, records)


# ---------------------------------------------------------------------------
# stream builders
# ---------------------------------------------------------------------------
def flow_rows(rng, nflows):
    return rng.integers(1, 256, (nflows, KF), dtype=np.uint8)


def stream(rng, flows, n, weights=None):
    """n packets over `flows` (uniform, or by weight), every element new."""
    p = None if weights is None else np.asarray(weights, np.float64) / np.sum(weights)
    fl = np.ascontiguousarray(flows[rng.choice(len(flows), n, p=p)])
    el = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.uint8).reshape(n, KE)
    return fl, np.ascontiguousarray(el)


def natural(name, seed, w, d, m, size, base, b, nflows, n, resets=0, weights=None, need=None):
    rng = np.random.default_rng(seed)
    flows = flow_rows(rng, nflows)
    sc = Scenario(name, w, d, m, size, base, b, need=need or {}, flows=flows)
    for part in range(resets + 1):
        if part:
            sc.ops.append(("reset",))
        sc.ops.append(("insert",) + stream(rng, flows, n // (resets + 1), weights))
    return sc


def crafted(name, seed, b=1.08, base=0.5, val=0, pbits=1.0, records=0, need=None, w=2, d=2, m=64, size=5, n=3000):
    """Flow 0 owns its cell of every row with counter `val`, every cell has the given pbits,
    registers empty, generator at `records`; then n packets, half from the owner and half from
    five others.  A key sits only in cells it hashes to, as in every state a stream can reach:
    the device's list takes a flow's max over the cells that hold it (gns_hh.hpp)."""
    rng = np.random.default_rng(seed)
    sc = Scenario(name, w, d, m, size, base, b, need=need or {})
    seeds = sc.seeds().tolist()

    def cells_of(f):
        return [i * w + pyref.mm3(bytes(f), s) % w for i, s in enumerate(seeds)]
    flows = [flow_rows(rng, 1)[0]]
    while len(flows) < 6:  # the others meet the owner in at least one row
        f = flow_rows(rng, 1)[0]
        if set(cells_of(f)) & set(cells_of(flows[0])):
            flows.append(f)
    sc.flows = flows = np.array(flows, np.uint8)
    cells = w * d
    values = np.zeros(cells, np.uint32)
    keys = np.zeros((cells, KF), np.uint8)
    if val:
        for c in cells_of(flows[0]):
            values[c], keys[c] = val, flows[0]
    regs = np.zeros((cells, m), np.uint8)
    pb = np.full(cells, pbits, np.float64)
    sc.ops.append(("import", values, keys, regs, pb, records))
    sc.ops.append(("insert",) + stream(rng, flows, n, [5, 1, 1, 1, 1, 1]))
    return sc


def crafted_again(name, seed, times, n, **kw):
    """crafted(), then the same import and another n packets `times` times over: as many
    first steps on a counter at exactly `val`."""
    sc = crafted(name, seed, n=n, **kw)
    rng = np.random.default_rng(seed + 1000)
    for _ in range(times - 1):
        sc.ops.append(sc.ops[0])
        sc.ops.append(("insert",) + stream(rng, sc.flows, n, [5, 1, 1, 1, 1, 1]))
    return sc


def mixed_chains(name, seed, w=4, d=2, n_heavy=4000, n_cold=40):
    """One call whose cells (all lanes of one wave) have chains on both sides of kSsLongChain:
    three heavy flows and three more share their cells, and a cold tail of flows, n_cold <= 48
    packets in all, hashes in at least one row to a cell none of the others uses, so that cell's
    chain stays short while the shared cells' chains run to hundreds of encodes."""
    rng = np.random.default_rng(seed)
    sc = Scenario(name, w, d, 256, 8, 0.5, 1.08, mixed=True, need={"foreign": 10, "decrement": 10})
    seeds = sc.seeds().tolist()

    def cells_of(f):
        return {i * w + pyref.mm3(bytes(f), s) % w for i, s in enumerate(seeds)}
    busy, used, cold = [], set(), []
    while len(busy) < 6:  # the busy flows leave at least one cell of the table unused
        f = flow_rows(rng, 1)[0]
        if len(used | cells_of(f)) < w * d:
            busy.append(f)
            used |= cells_of(f)
    while len(cold) < 4:
        f = flow_rows(rng, 1)[0]
        if cells_of(f) - used:
            cold.append(f)
    sc.flows = np.array(busy + cold, np.uint8)
    fb, eb = stream(rng, sc.flows[:6], n_heavy, [30, 20, 10, 2, 2, 2])
    fc, ec = stream(rng, sc.flows[6:], n_cold)
    order = rng.permutation(n_heavy + n_cold)
    sc.ops.append(("insert", np.ascontiguousarray(np.concatenate([fb, fc])[order]),
                   np.ascontiguousarray(np.concatenate([eb, ec])[order])))
    return sc


def chain_stream(seed=41, n=1500):
    rng = np.random.default_rng(seed)
    flows = flow_rows(rng, 12)
    return flows, stream(rng, flows, n, [12] + [1] * 11)


def chain_case(L):
    """The single-cell m = 256, size = 8 geometry, cut where the cell's L-th encode happens:
    the first call's chain is exactly L encodes, the second call holds the rest."""
    flows, (fl, el) = chain_stream()
    sc = Scenario(f"chain_{L}", 1, 1, 256, 8, 0.5, 1.08, flows=flows, chain=L,
                  need={"encode": L, "foreign": 10})
    if "cuts" not in _cache:  # one census pass: the packet after which the cell has had L encodes
        c, cuts = sc.census(), {}
        for i in range(len(fl)):
            c.insert(bytes(fl[i]), bytes(el[i]))
            cuts.setdefault(c.counts["encode"], i + 1)  # w = d = 1: at most one encode per packet
        _cache["cuts"] = cuts
    cut = _cache["cuts"].get(L)
    assert cut is not None, f"the stream has fewer than {L} encodes"
    sc.ops = [("insert", fl[:cut], el[:cut]), ("insert", fl[cut:], el[cut:])]
    return sc


def _scenarios():
    S = []
    # -- natural streams ------------------------------------------------------------------
    # m = 1 / 2, size = 3: a cell saturates, pbits reaches 0.0 exactly, -1.0 after the next reset
    S.append(natural("m1_size3_resets", 1, 4, 1, 1, 3, 0.5, 1.08, 6, 3200, resets=3,
                     need={"tempP_zero": 1, "tempP_neg": 10, "tempP_lt_m1": 1, "real_at_m1": 1, "lz_sat": 1,
                           "vv_nonpos": 10}))
    S.append(natural("m2_size3_b2_resets", 2, 8, 1, 2, 3, 0.5, 2.0, 10, 3200, resets=2,
                     need={"tempP_zero": 1, "tempP_neg": 10, "lz_sat": 10, "vv_nonpos": 10}))
    S.append(natural("size1_m8", 3, 4, 2, 8, 1, 0.5, 1.08, 8, 1600, resets=2,
                     need={"lz_sat": 10, "tempP_zero": 1, "tempP_neg": 10}))
    S.append(natural("size2_m100", 4, 5, 2, 100, 2, 0.5, 1.08, 20, 3000,
                     need={"lz_sat": 10, "foreign": 10, "decrement": 10}))
    S.append(natural("m256_one_cell", 5, 1, 1, 256, 8, 0.5, 1.08, 12, 6000, weights=[3, 2, 2] + [1] * 9,
                     need={"foreign": 10, "decrement": 10, "takeover_after_dec": 10, "draw_later": 10,
                           "wait_past": 10}))
    S.append(natural("m3_d8", 6, 2, 8, 3, 5, 0.5, 1.08, 10, 2000, need={"foreign": 10, "decrement": 10}))
    S.append(natural("b_1.0", 7, 4, 2, 64, 5, 0.5, 1.0, 12, 3000, need={"ppp_ge1": 10, "takeover_after_dec": 10}))
    S.append(natural("b_0.9", 8, 4, 2, 64, 5, 0.5, 0.9, 12, 3000, need={"ppp_ge1": 10, "takeover_after_dec": 10}))
    S.append(natural("b_1e6", 9, 2, 2, 256, 8, 0.5, 1e6, 8, 3000, weights=[8] + [1] * 7,
                     need={"ppp_zero": 10, "ppp_series": 10, "ppp_subnormal": 1}))
    S.append(natural("b_2.0", 10, 1, 1, 256, 8, 0.5, 2.0, 6, 4000, weights=[5] + [1] * 5,
                     need={"ppp_zero": 10, "ppp_series": 10, "ppp_subnormal": 1}))
    # one wave holding several long chains and short ones
    S.append(mixed_chains("w4_d2_m256_mixed", 11))
    # -- crafted states -------------------------------------------------------------------
    S.append(crafted("val_wrap", 20, val=0xFFFFFF00, need={"wrap": 1, "foreign_val_2048": 10, "ppp_zero": 10}))
    for v in (2047, 2048, 2049, 3000, 9000):
        S.append(crafted(f"val_{v}", 21 + v, val=v, need={"foreign_val_2048": 10, "ppp_series": 10, "wait_past": 10}))
    # val exactly kSsMvTab where the step does decrement: b <= 1, and b so close to 1 that b^-2048 = 0.13
    S.append(crafted_again("b1.0_val_2048", 46, 10, 200, b=1.0, val=2048,
                           need={"decrement_at_2048": 1, "foreign_val_2048": 10}))
    S.append(crafted_again("b1.001_val_2048", 47, 10, 200, b=1.001, val=2048,
                           need={"decrement_at_2048": 1, "foreign_val_2048": 10, "decrement": 10}))
    S.append(crafted("val_9600", 30, val=9600, need={"foreign_val_2048": 10, "ppp_subnormal": 10, "ppp_zero": 10}))
    S.append(crafted("val_9700", 31, val=9700, need={"foreign_val_2048": 10, "ppp_zero": 10}))
    S.append(crafted("b2_val_1000", 32, b=2.0, val=1000, need={"ppp_subnormal": 10, "ppp_series": 10, "ppp_zero": 10}))
    S.append(crafted("b2_val_1070", 33, b=2.0, val=1070, need={"ppp_subnormal": 1, "ppp_zero": 10}))
    S.append(crafted("b0.5_val_2000", 34, b=0.5, val=2000, need={"ppp_ge1": 10, "foreign_val_2048": 10}))
    # b <= 1 at the largest counter: b^-val is +inf / 1, the step decrements (a "no value yet"
    # marker of 2^32 - 1 in the walk's b^-val memo once took this for a known underflow)
    S.append(crafted("b0.9_val_max", 44, b=0.9, val=0xFFFFFFFF, need={"foreign_val_max": 1, "ppp_ge1": 10}))
    S.append(crafted("b1.0_val_max", 45, b=1.0, val=0xFFFFFFFF, need={"foreign_val_max": 1, "ppp_ge1": 10}))
    S.append(crafted("pbits_2pow-40", 35, pbits=2.0 ** -40, need={"vv_big": 1, "wrap": 1, "tempP_neg": 10}))
    S.append(crafted("pbits_2pow-36_val_300", 36, pbits=2.0 ** -36, val=300,
                     need={"vv_big": 1, "draw_later": 10, "decrement": 10}))
    S.append(crafted("pbits_1e-300", 37, pbits=1e-300, need={"vv_nonpos": 10, "tempP_neg": 10}))
    S.append(crafted("pbits_5e-324", 38, pbits=5e-324, need={"vv_nonpos": 10, "tempP_neg": 10}))
    S.append(crafted("pbits_0", 39, pbits=0.0, need={"tempP_zero": 1, "tempP_neg": 10, "vv_nonpos": 10}))
    S.append(crafted("pbits_-1", 40, pbits=-1.0, need={"real_at_m1": 1, "tempP_lt_m1": 10}))
    S.append(crafted("pbits_-0.875", 41, pbits=-0.875, need={"tempP_neg": 10, "tempP_lt_m1": 10, "vv_nonpos": 10}))
    S.append(crafted("records_2pow63", 42, records=2**63 - 100, need={"foreign": 10, "decrement": 10}))
    S.append(crafted("records_2pow32", 43, records=2**32 - 50, need={"foreign": 10, "decrement": 10}))
    # -- chain lengths --------------------------------------------------------------------
    S += [chain_case(L) for L in CHAIN_L]
    return S


_cache = {}


def scenarios():
    if "S" not in _cache:
        _cache["S"] = _scenarios()
    return _cache["S"]


def names():
    return [s.name for s in scenarios()]


def by_name(name):
    return next(s for s in scenarios() if s.name == name)


def reference(sc, ragged):
    """The census run of a scenario, once per (scenario, split): the states after every
    call, the regime counts and the chains.  Shared and never modified."""
    key = (sc.name, ragged)
    if key not in _cache:
        c = sc.census()
        states, encodes = [], []
        for op in sc.calls(ragged):
            apply(c, op)
            states.append(c.export())
            encodes.append(c.counts["encode"])
        _cache[key] = (states, encodes, c.counts, c.chain)
    return _cache[key]
