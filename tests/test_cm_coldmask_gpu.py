"""K3s takes its sub-passes over the packets K1's cold mask marks (inserted, with
at least one row that is not a designated bucket).  Every case compares the
exported device state (C, S, both fingerprint arrays) bit-exact with the
sequential C oracle fed the same stream, at the block shapes where the cold list
changes path: no cold packet, all cold, 8191 / 8192 / 8193 cold packets in a K1
block of 16384, mixed rows, records that are not inserted, the 512-bin kernel."""
import numpy as np
import pytest

from helpers import frames_from_tuples, random_tuples, sizes_u32, zipf_keys

pytestmark = pytest.mark.gpu

BLOCK = 16384  # packets per K1 / K3s block
SUB = 8192     # cold packets per K3s sub-pass
HOT_MIN = 1024  # a bucket is designated only with C >= 1024
HOT_PER_ROW = 128


def assert_same_state(cm, orc):
    for name, a, b in zip(("C", "S", "FPc", "FPs"), cm.export_state(), orc.export()):
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0] if a.ndim == 1 else np.nonzero((a != b).any(axis=1))[0]
            raise AssertionError(f"{name} differs in {len(bad)} cells, first {bad[:5]}: "
                                 f"gpu={a[bad[:3]]} oracle={b[bad[:3]]}")


def make_pair(oracle, w, d, K, seed=1, **kw):
    from go2netspectra_amd import CountMin
    seeds = np.random.default_rng(seed).integers(0, 2**32, d, dtype=np.uint64).astype(np.uint32)
    return CountMin(w, d, 1000, 10, key_bytes=K, seeds=seeds, **kw), oracle.CountMin(w, d, 1000, 10, K, seeds), seeds


def insert_both(cm, orc, keys, sizes):
    cm.insert_keys(keys, sizes)
    cm.flush()
    orc.insert_keys(keys, sizes)


def rows_of(orc, d):
    return np.asarray(orc.export()[0]).reshape(d, -1)


def test_blocks_with_no_cold_packet(gpu, oracle):
    """100 flows with exactly 1000 packets each per call of 100,000.  A bucket is designated
    from C >= 1024, which 100 flows cannot all reach in 100,000 packets, so the premise is
    taken where it can hold: after the second call every bucket in use has C = 2000 and
    there are at most 128 per row, so every one is designated and the third call's seven
    K1 blocks carry no cold packet (the second call's carry only cold ones)."""
    rng = np.random.default_rng(41)
    w, d, K = 1 << 16, 4, 16
    cm, orc, _ = make_pair(oracle, w, d, K)
    flows = rng.integers(0, 256, (100, K), dtype=np.uint8)
    assert len(np.unique(flows, axis=0)) == 100
    for call in range(3):
        keys = np.ascontiguousarray(flows[rng.permutation(np.repeat(np.arange(100), 1000))])
        insert_both(cm, orc, keys, sizes_u32(rng, 100_000))
        C = rows_of(orc, d)
        assert ((C != 0).sum(axis=1) <= HOT_PER_ROW).all()
        if call >= 1:
            assert (C[C != 0] >= HOT_MIN).all()
        assert_same_state(cm, orc)


def test_blocks_that_are_all_cold(gpu, oracle):
    """Uniform packets over 200,000 flows: every packet is cold, so a full block takes two
    full sub-passes and the last block has 37 packets (one partial mask word)."""
    rng = np.random.default_rng(42)
    cm, orc, _ = make_pair(oracle, 1 << 20, 4, 37)
    n = 3 * BLOCK + 37
    flows = rng.integers(0, 256, (200_000, 37), dtype=np.uint8)
    keys = np.ascontiguousarray(flows[rng.integers(0, 200_000, n)])
    insert_both(cm, orc, keys, sizes_u32(rng, n))
    assert (rows_of(orc, 4) < HOT_MIN).all()
    assert_same_state(cm, orc)


@pytest.mark.parametrize("d", [1, 2])
def test_all_cold_shallow(gpu, oracle, d):
    """Two sub-passes per block at depths 1 and 2, where the step that expands the next
    sub-pass's offsets is the block's first (d = 2) or every step is a last row (d = 1)."""
    rng = np.random.default_rng(47 + d)
    cm, orc, _ = make_pair(oracle, 1 << 20, d, 16)
    n = 2 * BLOCK + 100
    flows = rng.integers(0, 256, (200_000, 16), dtype=np.uint8)
    keys = np.ascontiguousarray(flows[rng.integers(0, 200_000, n)])
    insert_both(cm, orc, keys, sizes_u32(rng, n))
    assert_same_state(cm, orc)


def test_sub_pass_boundary(gpu, oracle):
    """64 designated heavy flows, then K1 blocks with exactly 8191, 8192 and 8193 packets of
    new one-packet flows at random positions: one sub-pass short by one, one exactly full,
    and a second sub-pass of a single packet.  The new flows are parked by K1 and get their
    ids from k_resolve after the mask was written."""
    rng = np.random.default_rng(43)
    w, d, K = 1 << 20, 4, 37
    cm, orc, _ = make_pair(oracle, w, d, K)
    heavy = rng.integers(0, 256, (64, K), dtype=np.uint8)
    heavy[:, 2] = 0x11  # (the new flows below carry 0xEE there)
    warm = np.ascontiguousarray(heavy[rng.integers(0, 64, 200_000)])
    insert_both(cm, orc, warm, sizes_u32(rng, 200_000))
    C = rows_of(orc, d)
    assert ((C >= HOT_MIN).sum(axis=1) == 64).all()
    ncold = (SUB - 1, SUB, SUB + 1)
    fresh = rng.integers(0, 256, (sum(ncold), K), dtype=np.uint8)
    fresh[:, 0] = np.arange(sum(ncold)) & 0xFF  # distinct: a counter in the first three bytes
    fresh[:, 1] = (np.arange(sum(ncold)) >> 8) & 0xFF
    fresh[:, 2] = 0xEE
    keys = np.ascontiguousarray(heavy[rng.integers(0, 64, 3 * BLOCK)])
    used = 0
    for b, c in enumerate(ncold):
        pos = b * BLOCK + rng.choice(BLOCK, c, replace=False)
        keys[pos] = fresh[used:used + c]
        used += c
    insert_both(cm, orc, keys, sizes_u32(rng, 3 * BLOCK))
    assert_same_state(cm, orc)


def test_mixed_rows(gpu, oracle):
    """A narrow sketch: tail flows keep colliding with designated buckets, so packets have
    some rows designated and some cold (their mask bit is set; K3s skips the hot rows)."""
    rng = np.random.default_rng(44)
    cm, orc, _ = make_pair(oracle, 256, 4, 16, batch_packets=65536)
    keys, _, _ = zipf_keys(rng, 300_000, 5000, 16)
    insert_both(cm, orc, keys, sizes_u32(rng, 300_000))
    assert_same_state(cm, orc)


def test_records_that_are_not_inserted(gpu, oracle):
    """The header path with VLAN tags and IPv6: dropped and unsupported records give mask
    bit 0 in the middle of a word."""
    from go2netspectra_amd import CountMin
    fields = ["SrcIP", "DstIP", "SrcPort", "DstPort", "Protocol"]
    rng = np.random.default_rng(45)
    n = 100_000
    t = random_tuples(rng, n, 3000, v6_frac=0.2)
    hdr = frames_from_tuples(t, rng, vlan_frac=0.3)
    seeds = np.array([0x1111, 0x2222, 0x3333, 0x4444], np.uint32)
    cm = CountMin(1 << 20, 4, 10_000, 30, flow_fields=fields, seeds=seeds)
    cm.insert_headers(hdr, t["length"])
    cm.flush()
    orc = oracle.CountMin(1 << 20, 4, 10_000, 30, 37, seeds)
    done = orc.insert_hdr64(hdr, t["length"], fields)
    st = cm.stats()
    assert st["inserted"] == done
    assert done == n - st["unsupported"] - st["dropped"]
    assert_same_state(cm, orc)


def test_512_bin_rows(gpu, oracle):
    """w = 2^21, d = 8: rows of 512 bins, the kernel with packed 16-bit counters."""
    rng = np.random.default_rng(46)
    cm, orc, _ = make_pair(oracle, 1 << 21, 8, 37)
    flows = rng.integers(0, 256, (300_000, 37), dtype=np.uint8)
    from helpers import zipf_index
    for _ in range(2):
        keys = np.ascontiguousarray(flows[zipf_index(rng, 200_000, 300_000)])
        insert_both(cm, orc, keys, sizes_u32(rng, 200_000))
    assert_same_state(cm, orc)
