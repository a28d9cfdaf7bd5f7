"""The truth side of the heavy-hitter history's retention tests, on top of HeavyTruth
(heavy_history_truth.py); nothing here comes from the engine.

    dropped(tr, before)  the reference's table after the partitions below `before` are dropped:
                         the rows with Timestamp < before are gone, and so are their snapshots
    folded(tr, before)   per (Type, Flow) the latest expired row, re-stamped to the last expired
                         time, plus every later row: one base snapshot in place of the expired ones

Rows keep their order, so the rows of one type are, in order, that type's log.  The fold also has
a statement that does not go through folded(): every answer at T >= the last expired time equals
the untrimmed table's (assert_fold_keeps_answers).  Point queries: point(tr, type, flow, T)."""
from heavy_history_truth import HeavyTruth


def _like(tr, rows, times):
    out = HeavyTruth(decode=tr.decode)
    out.rows, out.times, out.bytes = list(rows), list(times), dict(tr.bytes)
    return out


def dropped(tr, before):
    return _like(tr, [r for r in tr.rows if r[0] >= before], [t for t in tr.times if t >= before])


def folded(tr, before):
    expired = [t for t in tr.times if t < before]
    if not expired:
        return _like(tr, tr.rows, tr.times)
    last = expired[-1]
    newest = {}  # (type, flow) -> index of its latest expired row
    for i, (ts, ty, s, v) in enumerate(tr.rows):
        if ts < before and ((ty, s) not in newest or ts > tr.rows[newest[ty, s]][0]):
            newest[ty, s] = i
    keep = set(newest.values())
    rows = [(last, ty, s, v) for i, (ts, ty, s, v) in enumerate(tr.rows) if i in keep]
    rows += [r for r in tr.rows if r[0] >= before]
    return _like(tr, rows, [last] + [t for t in tr.times if t >= before])


def trimmed(tr, before, fold):
    return folded(tr, before) if fold else dropped(tr, before)


def trim_out(tr, before, fold):
    """What gns_hh_hist_trim reports: snapshots removed, rows removed, pairs forgotten, rows left."""
    after = trimmed(tr, before, fold)
    pairs = lambda t: {(ty, s) for _, ty, s, _ in t.rows}
    return [len(tr.times) - len(after.times), len(tr.rows) - len(after.rows), len(pairs(tr) - pairs(after)), len(after.rows)]


def assert_fold_keeps_answers(tr, ftr, types):
    """The independent statement of a fold: at and after the base's time nothing changed; before it, nothing is left."""
    if not ftr.times:
        return
    base = ftr.times[0]
    for T in tr.probe_times():
        for type in types:
            if T is None or T >= base:
                assert ftr.query(type, end_time=T) == tr.query(type, end_time=T), (type, T)
            else:
                assert ftr.query(type, end_time=T) == [], (type, T)


def point(tr, type, flow, T=None):
    """The value of the live row of (type, flow bytes) as of T, None without one."""
    return tr.latest(type, T).get(tr.decode(bytes(flow)))


def log_of(tr, type):
    """[(written, flow bytes, value)] of one type in log order."""
    num = {t: i for i, t in enumerate(tr.times)}
    return [(num[ts], tr.bytes[s], v) for ts, ty, s, v in tr.rows if ty == type]
