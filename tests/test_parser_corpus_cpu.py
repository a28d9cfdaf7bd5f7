"""The record parser's boundary corpus (tests/parser_corpus.py) on the CPU: the C oracle
(or_parse_hdr64_len, the expected value of every GPU parser test), the independent
whole-frame restatement (oracle/pyframe.py) and the packer's escape record must agree
on every corpus record and on 20,000 mutants, with no record excluded.

A record with ethertype 0x88B5 is not a frame but the packer's pre-parsed form
(DESIGN.md §5); its expected tuple is the literal content of its fields."""
import struct
from collections import defaultdict

import pytest

import parser_corpus as pc
from oracle import pyframe


@pytest.fixture(scope="module")
def records():
    base = pc.corpus()
    return base, base + pc.mutants(20_000, base=base)


def literal_preparsed(rec: bytes):
    """0x88B5, kind 1, source version, src16, dst16, ports BE, protocol."""
    if rec[14] != 1:
        return None
    sp, dp, pr = struct.unpack_from(">HHB", rec, 48)
    return rec[16:32], rec[32:48], sp, dp, pr


def test_corpus_is_deterministic_and_named_once(records):
    base, allrec = records
    assert base == pc.corpus()
    assert allrec[len(base):len(base) + 50] == pc.mutants(50, base=base)
    assert len({name for name, _, _ in allrec}) == len(allrec)
    assert all(len(r) == 64 and 0 <= w < 2**32 for _, r, w in allrec)
    fh, fw = pc.filler_pool()
    assert all(pyframe.fast_shape(pc.frame_of(bytes(h), int(w)), int(w)) for h, w in zip(fh, fw))


def test_oracle_pyframe_and_escape_agree(oracle, records):
    base, allrec = records
    seen = defaultdict(set)
    fast = 0
    bad = []
    for name, rec, wl in allrec:
        st, src, dst, sp, dp, pr = oracle.parse_hdr64(rec, wl)
        got = (src, dst, sp, dp, pr)
        frame = pc.frame_of(rec, wl)
        ft = pyframe.frame_tuple(frame)
        pre = rec[12:14] == b"\x88\xb5"
        if pre:
            want = literal_preparsed(rec)
            if (st == 0) != (want is not None) or (st == 0 and got != want) or st == 1:
                bad.append((name, "preparsed", st, got, want))
        elif st == 0:
            if ft is None or got != ft[:5]:
                bad.append((name, "status 0", got, ft))
        elif st == 1:
            if ft is not None:
                bad.append((name, "status 1", ft))
        else:
            assert st == 2, name
        # the escape path: what the packer hands the device for this frame parses to the frame's tuple
        est, *esc = oracle.parse_hdr64(pyframe.frame_record(frame, wl), wl)
        if (est, tuple(esc)) != ((1, (bytes(16), bytes(16), 0, 0, 0)) if ft is None else (0, ft[:5])):
            bad.append((name, "escape", est, esc, ft))
        fast += pyframe.fast_shape(frame, wl)
        nil = st == 0 and not pre and ft is not None and ft[5] == 0
        seen[pc.group(name)].add({1: "drop", 2: "unsupported"}.get(st) or
                                 ("nil" if nil else "ports" if (sp or dp) else "noports"))
    assert not bad, f"{len(bad)} of {len(allrec)} records disagree; first: {bad[:5]}"
    assert fast > 100
    # each group holds both sides of its boundary
    want = {"v4_after_l2": {"drop", "nil", "noports", "ports", "unsupported"},
            "v4_total": {"noports", "ports", "unsupported"},
            "v4_ihl": {"noports", "ports", "unsupported"},
            "v4_frag": {"noports", "ports", "unsupported"},
            "ip_version": {"ports", "unsupported"},
            "v4_proto": {"noports", "ports", "unsupported"},
            "v6_nexthdr": {"noports", "ports", "unsupported"},
            "tunnel_port": {"ports", "unsupported"},
            "v6_after_l2": {"drop", "nil", "noports", "ports", "unsupported"},
            "ethertype": {"drop", "unsupported"},
            "short_wire": {"drop", "unsupported"},  # unsupported: the third tag alone
            "preparsed": {"noports", "ports", "unsupported"},
            "mutant": {"drop", "nil", "noports", "ports", "unsupported"}}
    assert {g: seen[g] for g in want} == want
    assert set(seen) == set(want)


def test_orderings_hold_every_record_once(records):
    base, _ = records
    hdr, wl = pc.to_arrays(base)
    fh, fw = pc.filler_pool()
    for name, (oh, ow, origin) in pc.orderings(hdr, wl).items():
        own = origin >= 0
        assert sorted(origin[own].tolist()) == list(range(len(wl))), name
        assert (oh[own] == hdr[origin[own]]).all() and (ow[own] == wl[origin[own]]).all(), name
        assert (oh[~own] == fh[-1 - origin[~own]]).all() and (ow[~own] == fw[-1 - origin[~own]]).all(), name
    _, _, o = pc.orderings(hdr, wl)["lane"]
    lanes = np_lanes(o)
    assert set(lanes) == set(pc.BALLOT_LANES) and len(o) == 64 * len(wl)
    _, _, o = pc.orderings(hdr, wl)["tail"]
    assert (o[:256] < 0).all() and (o[-(len(wl) % 100 or 100):] >= 0).all()
    starts = [i for i in range(len(o)) if o[i] >= 0 and (i == 0 or o[i - 1] < 0)]
    assert all(s % 256 == 0 for s in starts)


def np_lanes(origin):
    return [i % 64 for i in range(len(origin)) if origin[i] >= 0]
