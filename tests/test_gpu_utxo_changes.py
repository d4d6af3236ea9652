"""Per-script changes of a journaled diff, read from the device undo journal
and the live table: kv_utxo_changes_by_spk ⇔ UtxoIndexChanges::update_utxo_diff
(indexes/utxoindex/src/update_container.rs:29-51) filtered as
UtxosChangedNotification::apply_utxos_changed_subscription does
(indexes/core/src/notification.rs:81-127), with the supply change of
indexes/utxoindex/src/index.rs:98.

The model is a Python dict outpoint -> Entry and a Python diff, independent of
the engine: which entries left and entered the set, under which change index,
and their 96-byte records are worked out here. Helpers are local, in the style
of test_gpu_utxo_query.py. Tables have 1,024 to 4,096 slots."""
import ctypes
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
from workload import gen_block  # noqa: E402

from rusty_kaspa_amd.blob import strip_utxo_entries  # noqa: E402

pytestmark = pytest.mark.gpu

F_COINBASE, F_ARENA, F_COVENANT, F_REMOVED = 1, 2, 4, 0x8000
REVERSED, ALL = 1, 2
MAX_SPK, QUERY_MAX, REC = 10000, 65536, 96
NO_QUERY = 0xFFFFFFFF
M64 = (1 << 64) - 1
SKIP_MASS = 2
TOTALS = ("cursor_end", "added_amount", "removed_amount", "n_added", "n_removed",
          "n_added_gone")


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


# ---------------- the independent model ----------------

class Entry:
    __slots__ = ("amount", "daa", "coinbase", "version", "spk", "cov")

    def __init__(self, amount, daa, spk, version=0, coinbase=False, cov=None):
        self.amount, self.daa, self.spk = amount, daa, spk
        self.version, self.coinbase, self.cov = version, coinbase, cov

    def flags(self):
        return (F_COINBASE if self.coinbase else 0) | (F_COVENANT if self.cov else 0)

    def in_blob(self):
        return self.cov is not None or len(self.spk) > 36

    def pack(self):
        """the 64-byte record handed to kv_utxo_upsert_spk / kv_utxo_apply_diff"""
        head = struct.pack("<QQHHI", self.amount, self.daa, self.flags(),
                           self.version, len(self.spk))
        if self.cov is not None:
            field = bytes(4) + self.cov
        elif len(self.spk) > 36:
            field = bytes(36)
        else:
            field = self.spk.ljust(36, b"\0")
        return head + field + bytes(4)

    def change(self, op36, query_index, removed):
        """the 96-byte change record of kv_utxo_changes_by_spk"""
        return (op36 + struct.pack("<IQQHHI", query_index, self.amount, self.daa,
                                   self.flags() | (F_REMOVED if removed else 0),
                                   self.version, len(self.spk))
                + (self.cov or bytes(32)))


def applied(before, removed, added):
    after = {op: e for op, e in before.items() if op not in set(removed)}
    after.update(added)
    return after


def model_changes(before, removed, added, queries, flags=0, now=None):
    """What the record of the diff (removed, added), applied to `before`, must
    report when the table holds `now` (default: the set right after the diff):
    ([(change index, record, script)] ascending, totals). `queries` is a list
    of (version, script), ignored under ALL."""
    now = applied(before, removed, added) if now is None else now
    index = None if flags & ALL else {q: i for i, q in enumerate(queries)}
    tot = dict.fromkeys(TOTALS, 0)
    tot["cursor_end"] = len(removed) + 2 * len(added)
    out = []

    def emit(c, op, e, left_the_set):
        label_removed = left_the_set != bool(flags & REVERSED)
        side = "removed" if label_removed else "added"
        tot[side + "_amount"] = (tot[side + "_amount"] + e.amount) & M64
        tot["n_" + side] += 1
        qi = NO_QUERY if index is None else index.get((e.version, e.spk))
        if qi is not None:
            out.append((c, e.change(op, qi, label_removed), e.spk))

    for c, op in enumerate(removed):
        if op in before:
            emit(c, op, before[op], True)
    for k, (op, _) in enumerate(added):
        c = len(removed) + 2 * k
        if op in before:
            emit(c, op, before[op], True)
        if op in now:
            emit(c + 1, op, now[op], False)
        else:
            tot["n_added_gone"] += 1
    return out, tot


# ---------------- table and journal helpers ----------------

def ctx(engine):
    return ctypes.c_void_p(engine.ctx)


def err(engine):
    return engine.lib.kv_last_error().decode()


def reset(engine, capacity):
    assert engine.lib.kv_utxo_reset(ctx(engine), ctypes.c_uint64(capacity)) == 0


def chunk_args(items):
    return (b"".join(op for op, _ in items), b"".join(e.pack() for _, e in items),
            b"".join(e.spk for _, e in items if e.in_blob()))


def upsert(engine, items):
    ops, ents, blob = chunk_args(items)
    rc = engine.lib.kv_utxo_upsert_spk(ctx(engine), ops, ents, blob,
                                       ctypes.c_size_t(len(blob)),
                                       ctypes.c_size_t(len(items)))
    assert rc == 0, err(engine)


def load(engine, capacity, items):
    reset(engine, capacity)
    upsert(engine, items)
    return dict(items)


def apply(engine, removed, added):
    token, _ = engine.utxo_apply_diff(b"".join(removed), *chunk_args(added))
    return token


def lookup(engine, ops):
    """[(found, entry64 with the script field blanked, script)] through the
    existing kv_utxo_lookup_spk"""
    n = len(ops)
    out = (ctypes.c_uint8 * (64 * n))()
    bm = (ctypes.c_uint64 * ((n + 63) // 64))()
    spk = (ctypes.c_uint8 * (1 << 16))()
    used = ctypes.c_size_t()
    rc = engine.lib.kv_utxo_lookup_spk(ctx(engine), b"".join(ops), ctypes.c_size_t(n),
                                       out, bm, spk, ctypes.c_size_t(1 << 16),
                                       ctypes.byref(used))
    assert rc == 0, err(engine)
    res = []
    for i in range(n):
        if not (bm[i // 64] >> (i % 64)) & 1:
            res.append(None)
            continue
        rec = bytes(out[64 * i:64 * (i + 1)])
        amount, daa, flags, ver, ln = struct.unpack_from("<QQHHI", rec)
        if flags & F_ARENA:
            off, = struct.unpack_from("<I", rec, 24)
            script = bytes(spk[off:off + ln])
        else:
            script = rec[24:24 + ln]
        cov = rec[28:60] if flags & F_COVENANT else None
        res.append((amount, daa, flags & ~F_ARENA, ver, script, cov))
    return res


def check_table(engine, model, absent=()):
    ops = list(model)
    want = [(e.amount, e.daa, e.flags(), e.version, e.spk, e.cov)
            for e in model.values()]
    assert lookup(engine, ops) == want
    absent = [op for op in absent if op not in model]
    if absent:
        assert lookup(engine, absent) == [None] * len(absent)
    assert engine.utxo_stats()["n_live"] == len(model)


def rand_op(rng):
    return rng.randbytes(32) + struct.pack("<I", rng.randrange(8))


def totals(res):
    return {k: res[k] for k in TOTALS}


class Walk:
    """a walk over one record: .records and .scripts in the order they came
    out, .sizes[i] the record count of call i, .totals what every call said"""

    def __init__(self, engine, token, queries, max_entries, flags=0, spk_cap=0,
                 start=0):
        self.records, self.scripts, self.sizes = [], [], []
        self.totals = None
        cursor = start
        while True:
            recs, spks, after, res = engine.utxo_changes_by_spk(
                token, queries, max_entries, cursor=cursor, flags=flags,
                spk_cap=spk_cap)
            assert res["kernel_ms"] >= 0.0
            if self.totals is None:
                self.totals = totals(res)
            assert totals(res) == self.totals  # the same in every call
            n = len(recs) // REC
            assert len(recs) == n * REC and n <= max_entries
            assert cursor <= after <= res["cursor_end"]
            assert after > cursor or cursor == res["cursor_end"]
            chunk = [recs[REC * i:REC * (i + 1)] for i in range(n)]
            self.records += chunk
            self.sizes.append(n)
            if spk_cap:
                at = 0
                for rec in chunk:
                    ln, = struct.unpack_from("<I", rec, 60)
                    self.scripts.append(spks[at:at + ln])
                    at += ln
                assert at == len(spks) <= spk_cap
            else:
                assert spks is None
            cursor = after
            if cursor == res["cursor_end"]:
                break
            assert n > 0, "a call that returned nothing did not end the walk"
        self.calls = len(self.sizes)


def check_one_call(engine, token, want, tot, queries, flags=0, scripts=False):
    """one call with max_entries larger than the answer"""
    walk = Walk(engine, token, queries, len(want) + 5, flags,
                spk_cap=MAX_SPK + sum(len(s) for _, _, s in want) if scripts else 0)
    assert walk.calls == 1
    assert walk.totals == tot
    assert walk.records == [rec for _, rec, _ in want]  # byte-exact, in order
    if scripts:
        assert walk.scripts == [s for _, _, s in want]
    return walk


# ---------------- 1: shapes around the wave ----------------

@pytest.fixture(scope="module")
def shape_items():
    rng = random.Random(201)
    lens = [34] * 8 + [35] * 3 + [0, 1, 20, 36, 37, 64, 200]
    scripts = [(i % 2, rng.randbytes(ln)) for i, ln in enumerate(lens)]

    def items(n):
        out = []
        for k in range(n):
            version, spk = scripts[rng.randrange(len(scripts))]
            out.append((rand_op(rng), Entry(
                rng.randrange(1 << 50), rng.randrange(1 << 40), spk, version,
                rng.random() < 0.1, rng.randbytes(32) if k % 11 == 3 else None)))
        return out
    base, fresh = items(300), items(130)
    queries = scripts[::2] + [(0, rng.randbytes(34)), (5, scripts[0][1])]
    rng.shuffle(queries)
    return base, fresh, queries


@pytest.mark.parametrize("n_added", [0, 1, 64, 130])
@pytest.mark.parametrize("n_removed", [0, 1, 63, 64, 65])
def test_shapes_around_the_wave(engine, shape_items, n_removed, n_added):
    base, fresh, queries = shape_items
    before = load(engine, 1024, base)
    removed = [op for op, _ in base[:n_removed]]
    added = fresh[:n_added]
    token = apply(engine, removed, added)
    want, tot = model_changes(before, removed, added, queries)
    assert tot["cursor_end"] == n_removed + 2 * n_added
    assert (tot["n_removed"], tot["n_added"]) == (n_removed, n_added)
    if n_removed + n_added >= 63:
        assert 0 < len(want) < n_removed + n_added  # about half the scripts
    check_one_call(engine, token, want, tot, queries)
    # the totals alone: no query, no record
    recs, spks, cursor, res = engine.utxo_changes_by_spk(token, [], 4)
    assert (recs, spks, cursor) == (b"", None, tot["cursor_end"])
    assert totals(res) == tot


# ---------------- 2: every script case in one diff ----------------

def script_entries(rng):
    """lengths 0, 1, 35, 36, 37, 200 and 10,000; abc against abc\\0; equal
    bytes under two versions; a covenant entry with a 5-byte script"""
    amount = lambda: rng.randrange(1, 1 << 50)
    daa = lambda: rng.randrange(1 << 40)
    s35, s5 = rng.randbytes(35), rng.randbytes(5)
    ents = [Entry(amount(), daa(), rng.randbytes(ln))
            for ln in (0, 1, 36, 37, 200, MAX_SPK)]
    ents += [
        Entry(amount(), daa(), s35),
        Entry(amount(), daa(), s35, version=1),          # equal bytes, version 1
        Entry(amount(), daa(), b"abc"),
        Entry(amount(), daa(), b"abc\0", coinbase=True),
        Entry(amount(), daa(), s5, cov=rng.randbytes(32)),  # arena, id carried
        Entry(amount(), daa(), s5),                      # the same script inline
        Entry(M64, daa(), rng.randbytes(34)),
    ]
    return [(rand_op(rng), e) for e in ents]


def test_every_script_case(engine):
    rng = random.Random(202)
    old, new = script_entries(rng), script_entries(rng)
    filler = [(rand_op(rng), Entry(rng.randrange(1 << 50), 7, rng.randbytes(34)))
              for _ in range(40)]
    before = load(engine, 512, old + filler)
    removed = [op for op, _ in old] + [op for op, _ in filler[:5]]
    added = new + [(rand_op(rng), Entry(9, 9, old[3][1].spk))]  # old 37-byte script
    token = apply(engine, removed, added)
    scripts = lambda items: [(e.version, e.spk) for _, e in items]
    present = list(dict.fromkeys(scripts(old) + scripts(new)))
    # every script of the diff but the fillers', and near misses of each kind
    queries = present + [(2, present[6][1]), (0, b"abc\0\0"), (0, b"ab"),
                         (0, present[5][1][:-1]), (0, rng.randbytes(34))]
    rng.shuffle(queries)
    want, tot = model_changes(before, removed, added, queries)
    assert len(want) == len(old) + len(new) + 1
    assert tot["n_removed"] == len(removed) and tot["n_added"] == len(added)
    by_q = {}
    for _, rec, _ in want:
        qi, = struct.unpack_from("<I", rec, 36)
        by_q[queries[qi]] = by_q.get(queries[qi], 0) + 1
    s5, s35 = old[10][1].spk, old[6][1].spk
    assert by_q[(0, s5)] == 2  # the covenant id is no key
    # one entry on each side of the diff for the scripts both sides share
    assert by_q[(0, b"abc")] == by_q[(0, b"abc\0")] == by_q[(0, b"")] == 2
    assert by_q[(0, s35)] == by_q[(1, s35)] == 1
    check_one_call(engine, token, want, tot, queries, scripts=True)
    # a subset of the queries: one at a time
    for q in [(0, s5), (1, s35), (0, b"abc"), (0, old[5][1].spk), (0, b"ab")]:
        w1, t1 = model_changes(before, removed, added, [q])
        assert t1 == tot
        check_one_call(engine, token, w1, tot, [q], scripts=True)
    # no filter: every entry, the fillers too, scripts the only way to know them
    want_all, tot_all = model_changes(before, removed, added, None, ALL)
    assert tot_all == tot and len(want_all) == len(removed) + len(added)
    walk = check_one_call(engine, token, want_all, tot, [], ALL, scripts=True)
    assert {len(s) for s in walk.scripts} >= {0, 1, 5, 35, 36, 37, 200, MAX_SPK}
    check_one_call(engine, token, want_all, tot, [], ALL)  # and without them


# ---------------- 3: every lane matches ----------------

def test_every_lane_matches(engine):
    rng = random.Random(203)
    hot = rng.randbytes(34)
    entry = lambda: Entry((1 << 57) - rng.randrange(1 << 20), rng.randrange(1 << 40),
                          hot)
    base = [(rand_op(rng), entry()) for _ in range(130)]
    fresh = [(rand_op(rng), entry()) for _ in range(130)]
    before = load(engine, 512, base)
    removed = [op for op, _ in base]
    token = apply(engine, removed, fresh)
    want, tot = model_changes(before, removed, fresh, [(0, hot)])
    assert len(want) == 260 and (tot["n_removed"], tot["n_added"]) == (130, 130)
    assert tot["removed_amount"] == sum(e.amount for _, e in base) & M64
    assert sum(e.amount for _, e in base) > M64  # the sum wraps
    check_one_call(engine, token, want, tot, [(0, hot)])
    many = [(0, struct.pack("<I", i) + bytes(30)) for i in range(999)]
    many.insert(617, (0, hot))
    want, tot2 = model_changes(before, removed, fresh, many)
    assert tot2 == tot and len(want) == 260
    assert {struct.unpack_from("<I", rec, 36)[0] for _, rec, _ in want} == {617}
    check_one_call(engine, token, want, tot, many)


# ---------------- 4: missing removes and overwriting adds ----------------

def mixed_items(rng, n, lens=(34, 34, 34, 35, 20, 37, 150)):
    return [(rand_op(rng), Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                                 rng.randbytes(rng.choice(lens)),
                                 coinbase=rng.random() < 0.1,
                                 cov=rng.randbytes(32) if k % 9 == 4 else None))
            for k in range(n)]


def test_missing_removes_and_overwriting_adds(engine):
    rng = random.Random(204)
    base = mixed_items(rng, 200)
    before = load(engine, 512, base)
    ghosts = [rand_op(rng) for _ in range(3)]
    removed = ghosts[:2] + [op for op, _ in base[:10]] + ghosts[2:]
    # overwrites: inline -> arena, arena -> inline, and the covenant entry
    over = [base[20][0], base[24][0], base[31][0]]
    added = mixed_items(rng, 6)
    added[1] = (over[0], Entry(5, 6, rng.randbytes(500)))
    added[3] = (over[1], Entry(7, 8, rng.randbytes(20)))
    added[4] = (over[2], Entry(9, 10, rng.randbytes(34)))
    token, res = engine.utxo_apply_diff(b"".join(removed), *chunk_args(added))
    assert (res["n_removed_missing"], res["n_added_overwrote"]) == (3, 3)
    want, tot = model_changes(before, removed, added, None, ALL)
    # the ghosts are neither reported nor summed
    assert tot["n_removed"] == 10 + 3 and tot["n_added"] == 6
    assert tot["removed_amount"] == sum(
        before[op].amount for op in removed[2:12] + over) & M64
    found = {c for c, _, _ in want}
    assert not found & {0, 1, 12}
    n_r = len(removed)
    for k in (1, 3, 4):  # the old value at the even index, the new one at + 1
        assert {n_r + 2 * k, n_r + 2 * k + 1} <= found
        old = next(rec for c, rec, _ in want if c == n_r + 2 * k)
        new = next(rec for c, rec, _ in want if c == n_r + 2 * k + 1)
        assert old[:36] == new[:36] == added[k][0]
        assert struct.unpack_from("<H", old, 56)[0] & F_REMOVED
        assert not struct.unpack_from("<H", new, 56)[0] & F_REMOVED
    for k in (0, 2, 5):
        assert n_r + 2 * k not in found and n_r + 2 * k + 1 in found
    check_one_call(engine, token, want, tot, [], ALL, scripts=True)
    queries = list(dict.fromkeys((e.version, e.spk) for e in before.values()))[::2]
    want_q, tot_q = model_changes(before, removed, added, queries)
    assert tot_q == tot
    check_one_call(engine, token, want_q, tot, queries, scripts=True)


# ---------------- 5: reversed, then the revert itself ----------------

def test_reversed_then_revert(engine):
    rng = random.Random(205)
    base = mixed_items(rng, 150)
    before = load(engine, 512, base)
    removed = [op for op, _ in base[:70]] + [rand_op(rng)]
    added = mixed_items(rng, 66)
    added[7] = (base[100][0], Entry(1, 2, rng.randbytes(60)))  # an overwrite
    token = apply(engine, removed, added)
    queries = list(dict.fromkeys(
        (e.version, e.spk) for _, e in base[:70:2] + added[::2] + [base[100]]))
    for flags, qs in ((0, queries), (ALL, [])):
        fwd = Walk(engine, token, qs, 500, flags, spk_cap=1 << 17)
        rev = Walk(engine, token, qs, 500, flags | REVERSED, spk_cap=1 << 17)
        want, tot = model_changes(before, removed, added, qs, flags | REVERSED)
        assert rev.records == [rec for _, rec, _ in want] and rev.totals == tot
        # the forward answer with the label bit flipped and the totals swapped
        flip = lambda rec: rec[:57] + bytes([rec[57] ^ 0x80]) + rec[58:]
        assert rev.records == [flip(rec) for rec in fwd.records] and fwd.records
        assert rev.scripts == fwd.scripts
        f, r = fwd.totals, rev.totals
        assert (r["added_amount"], r["removed_amount"], r["n_added"], r["n_removed"]) \
            == (f["removed_amount"], f["added_amount"], f["n_removed"], f["n_added"])
        assert (r["cursor_end"], r["n_added_gone"]) == (f["cursor_end"], 0)
        assert f["n_removed"] == 71 and f["n_added"] == 66
    check_table(engine, applied(before, removed, added), removed)
    engine.utxo_revert(token)
    check_table(engine, before, [op for op, _ in added])
    with pytest.raises(RuntimeError):
        engine.utxo_changes_by_spk(token, [], 4, flags=ALL)
    assert raw_changes(engine, token)[0] == -1


# ---------------- 6: pagination ----------------

def test_pagination(engine):
    rng = random.Random(206)
    base = mixed_items(rng, 200)
    before = load(engine, 512, base)
    removed = [op for op, _ in base[:90]]
    added = mixed_items(rng, 80)
    for k in (10, 11, 40):
        added[k] = (base[100 + k][0], added[k][1])  # overwrites: even indices exist
    token = apply(engine, removed, added)
    queries = list(dict.fromkeys(
        (e.version, e.spk) for _, e in base[:130:2] + added[::2]))
    queries += [(0, rng.randbytes(34)) for _ in range(3)]
    for flags, qs in ((0, queries), (ALL, [])):
        want, tot = model_changes(before, removed, added, qs, flags)
        one = check_one_call(engine, token, want, tot, qs, flags)
        assert len(want) > 64
        for max_entries in (1, 7, 64):
            walk = Walk(engine, token, qs, max_entries, flags)
            assert walk.records == one.records and walk.totals == tot
            assert walk.calls <= len(want) // max_entries + 1
            assert all(n == max_entries for n in walk.sizes[:-1])
        cs = [c for c, _, _ in want]
        assert cs == sorted(set(cs))  # strictly ascending
        # from a cursor in the middle: an even and an odd added index, both of
        # an overwritten row, and one past the last match
        n_r = len(removed)
        for start in (n_r + 2 * 10, n_r + 2 * 11 + 1, n_r + 2 * 40 + 1, 45,
                      cs[-1] + 1, tot["cursor_end"]):
            rest = [rec for c, rec, _ in want if c >= start]
            for max_entries in (7, 500):
                part = Walk(engine, token, qs, max_entries, flags, start=start)
                assert part.records == rest and part.totals == tot
        assert want[-1][0] < tot["cursor_end"]


def test_two_largest_scripts_come_one_per_call(engine):
    rng = random.Random(207)
    big = [(rand_op(rng), Entry(rng.randrange(1 << 50), 3, rng.randbytes(MAX_SPK)))
           for _ in range(2)]
    small = [(rand_op(rng), Entry(rng.randrange(1 << 50), 4, rng.randbytes(34)))
             for _ in range(3)]
    before = load(engine, 512, big + small[:1])
    removed = [op for op, _ in big + small[:1]]
    token = apply(engine, removed, small[1:])
    want, tot = model_changes(before, removed, small[1:], None, ALL)
    walk = Walk(engine, token, [], 64, ALL, spk_cap=MAX_SPK)
    assert walk.sizes == [1, 1, 3]
    assert walk.records == [rec for _, rec, _ in want]
    assert walk.scripts == [s for _, _, s in want] and walk.totals == tot
    # filtered to the two: still one per call
    qs = [(0, big[1][1].spk), (0, big[0][1].spk)]
    walk = Walk(engine, token, qs, 64, spk_cap=MAX_SPK)
    assert walk.sizes == [1, 1] and walk.scripts == [big[0][1].spk, big[1][1].spk]
    # without scripts nothing ends a chunk early
    assert Walk(engine, token, [], 64, ALL).sizes == [5]


# ---------------- 7: an older record, and a rehash in between ----------------

def test_older_record_and_rehash(engine):
    rng = random.Random(208)
    base = mixed_items(rng, 120)
    s0 = load(engine, 512, base)
    x = (rand_op(rng), Entry(123456, 77, rng.randbytes(200), coinbase=True))
    removed_a = [op for op, _ in base[:20]]
    added_a = mixed_items(rng, 15) + [x] + mixed_items(rng, 4)
    token_a = apply(engine, removed_a, added_a)
    s1 = applied(s0, removed_a, added_a)
    removed_b = [op for op, _ in base[30:40]] + [x[0]]
    added_b = mixed_items(rng, 12)
    token_b = apply(engine, removed_b, added_b)
    s2 = applied(s1, removed_b, added_b)
    # A, as the table is now: X is gone, everything else as A left it
    want_a, tot_a = model_changes(s0, removed_a, added_a, None, ALL, now=s2)
    assert tot_a["n_added_gone"] == 1 and tot_a["n_added"] == len(added_a) - 1
    assert not any(rec[:36] == x[0] for _, rec, _ in want_a)
    check_one_call(engine, token_a, want_a, tot_a, [], ALL, scripts=True)
    # B reports X removed, with the value A gave it
    want_b, tot_b = model_changes(s1, removed_b, added_b, [(0, x[1].spk)])
    assert [rec for _, rec, _ in want_b] == [x[1].change(x[0], 0, True)]
    assert tot_b["n_added_gone"] == 0
    check_one_call(engine, token_b, want_b, tot_b, [(0, x[1].spk)], scripts=True)
    want_b, _ = model_changes(s1, removed_b, added_b, None, ALL)
    answers = [(check_one_call(engine, t, w, tt, [], ALL, scripts=True).records)
               for t, w, tt in ((token_a, want_a, tot_a), (token_b, want_b, tot_b))]
    # slots and arena offsets move; the answers do not
    st = engine.utxo_stats()
    assert st["arena_used"] > st["arena_live_bytes"]  # X's script, for one
    engine.utxo_rehash(0)
    st = engine.utxo_stats()
    assert st["arena_used"] == st["arena_live_bytes"] and st["n_tomb"] == 0
    again = [(check_one_call(engine, t, w, tt, [], ALL, scripts=True).records)
             for t, w, tt in ((token_a, want_a, tot_a), (token_b, want_b, tot_b))]
    assert again == answers
    queries = [(e.version, e.spk) for _, e in added_a[::2]]
    want_q, tot_q = model_changes(s0, removed_a, added_a, queries, now=s2)
    check_one_call(engine, token_a, want_q, tot_q, queries, scripts=True)


# ---------------- 8: refusals ----------------

PATTERN = 0xA5


def raw_changes(engine, token, flags=0, cursor=0, heads=(), n_q=None, blob=b"",
                blob_len=None, max_entries=4, spk_cap=None, null=()):
    """(rc, untouched): the call through ctypes with every output preset to a
    pattern. spk_cap None: no spk_out. `null` names pointers passed as NULL."""
    from rusty_kaspa_amd.engine import KvSpkQuery, KvUtxoChangesResult
    arr = (KvSpkQuery * max(len(heads), 1))(*[KvSpkQuery(*h) for h in heads])
    out = (ctypes.c_uint8 * (REC * 4))(*[PATTERN] * (REC * 4))
    spk = (ctypes.c_uint8 * (2 * MAX_SPK))(*[PATTERN] * (2 * MAX_SPK))
    cur, n, used = ctypes.c_uint64(cursor), ctypes.c_size_t(PATTERN), \
        ctypes.c_size_t(PATTERN)
    res = KvUtxoChangesResult(*[PATTERN] * 6, -1.0)
    ptr = lambda name, obj: None if name in null else ctypes.byref(obj)
    rc = engine.lib.kv_utxo_changes_by_spk(
        ctx(engine), ctypes.c_uint64(token), ctypes.c_uint32(flags),
        ptr("cursor", cur), arr, ctypes.c_size_t(len(heads) if n_q is None else n_q),
        blob, ctypes.c_size_t(len(blob) if blob_len is None else blob_len),
        ctypes.c_size_t(max_entries), out, None if spk_cap is None else spk,
        ctypes.c_size_t(spk_cap or 0), ctypes.byref(used), ptr("n_out", n),
        ptr("res_out", res))
    untouched = (bytes(out) == bytes([PATTERN]) * (REC * 4)
                 and bytes(spk) == bytes([PATTERN]) * (2 * MAX_SPK)
                 and cur.value == cursor and n.value == used.value == PATTERN
                 and [getattr(res, f) for f, _ in res._fields_]
                 == [PATTERN] * 6 + [-1.0])
    return rc, untouched


def test_refusals_write_nothing(engine):
    rng = random.Random(209)
    base = mixed_items(rng, 60, lens=(34,))
    before = load(engine, 512, base)
    s34 = base[0][1].spk
    removed = [op for op, _ in base[:8]]
    token = apply(engine, removed, mixed_items(rng, 5, lens=(34,)))
    end = 8 + 2 * 5
    ok = dict(heads=[(34, 0, 0), (3, 0, 0)], blob=s34 + b"abc")
    cases = {
        "null cursor": dict(ok, null=("cursor",)),
        "null n_out": dict(ok, null=("n_out",)),
        "null res_out": dict(ok, null=("res_out",)),
        "max_entries 0": dict(ok, max_entries=0),
        "unknown flag 4": dict(ok, flags=4),
        "unknown flag high": dict(ok, flags=0x80000001),
        "ALL with a query": dict(ok, flags=ALL),
        "never issued": dict(ok, token=token + 100),
        "token 0": dict(ok, token=0),
        "cursor past the end": dict(ok, cursor=end + 1),
        "spk_cap below the limit": dict(ok, spk_cap=MAX_SPK - 1),
        "spk_cap below the limit, ALL": dict(flags=ALL, spk_cap=1),
        "duplicate": dict(heads=[(34, 0, 0), (3, 0, 0), (34, 0, 0)],
                          blob=s34 + b"abc" + s34),
        "over-long script": dict(heads=[(34, 0, 0), (MAX_SPK + 1, 0, 0)],
                                 blob=s34 + bytes(MAX_SPK + 1)),
        "too many queries": dict(heads=[(0, 0, 0)], n_q=QUERY_MAX + 1),
        "blob too long": dict(heads=[(34, 0, 0)], blob=s34 + b"\0"),
        "blob too short": dict(ok, blob_len=36),
        "non-zero zero field": dict(heads=[(34, 0, 0), (3, 0, 1)], blob=s34 + b"abc"),
        "ALL with a blob": dict(flags=ALL, blob=b"abc"),
    }
    for name, kw in cases.items():
        kw = dict(kw)
        assert raw_changes(engine, kw.pop("token", token), **kw) == (-1, True), name
        assert err(engine), name
    # the same arguments, mended, are served, at the end of the walk too
    assert raw_changes(engine, token, **ok) == (0, False)
    assert raw_changes(engine, token, cursor=end, **ok) == (0, False)
    assert raw_changes(engine, token, spk_cap=MAX_SPK, **ok) == (0, False)
    want, tot = model_changes(before, removed, [], [(0, s34), (0, b"abc")])
    recs, _, cursor, res = engine.utxo_changes_by_spk(token, [(0, s34), (0, b"abc")], 4)
    assert recs == want[0][1] and cursor == end and res["n_removed"] == 8
    # a dropped record, and every record after a reset
    token2 = apply(engine, [base[20][0]], [])
    engine.utxo_journal_drop(token)
    assert raw_changes(engine, token, **ok) == (-1, True)
    assert raw_changes(engine, token2, **ok) == (0, False)
    reset(engine, 512)
    assert raw_changes(engine, token2, **ok) == (-1, True)
    assert raw_changes(engine, token2, flags=ALL) == (-1, True)
    # an empty diff is a record like any other
    token3 = apply(engine, [], [])
    recs, spks, cursor, res = engine.utxo_changes_by_spk(token3, [], 4, flags=ALL,
                                                         spk_cap=MAX_SPK)
    assert (recs, spks, cursor) == (b"", b"", 0)
    assert totals(res) == dict.fromkeys(TOTALS, 0)


# ---------------- 9: a block through validation ----------------

def block_outputs(blob, n):
    """per tx of a populated blob: (tx_id, [(value, version, script, covenant id)])"""
    offs = list(struct.unpack_from(f"<{n}I", blob, 4))
    txs = []
    for off in offs:
        n_in, n_out = struct.unpack_from("<HH", blob, off + 2)
        payload_len, = struct.unpack_from("<I", blob, off + 36)
        tx_id = blob[off + 56:off + 88]
        p = off + 88 + payload_len
        for _ in range(n_in):
            sig_len, = struct.unpack_from("<I", blob, p + 48)
            p += 52 + sig_len
            has_cov = blob[p + 17]
            spk_len, = struct.unpack_from("<I", blob, p + 20)
            p += 24 + spk_len + (32 if has_cov else 0)
        outs = []
        for _ in range(n_out):
            value, version, _, spk_len = struct.unpack_from("<QHHI", blob, p)
            spk = blob[p + 16:p + 16 + spk_len]
            p += 16 + spk_len
            cov = None
            if blob[p]:
                cov = blob[p + 3:p + 35]
                p += 35
            else:
                p += 1
            outs.append((value, version, spk, cov))
        txs.append((tx_id, outs))
    return txs


def test_a_block_through_validation(engine, oracle):
    n, block_daa = 4, 10**9
    # seed 39: txs 0 and 2 are accepted, 1 and 3 carry a bad signature
    blob, _ = gen_block(oracle, seed=39, n_txs=n, pct_multi_input=50, pct_ecdsa=25,
                        pct_invalid=30)
    stripped, seeds = strip_utxo_entries(blob)
    offs = struct.unpack_from(f"<{n}I", blob, 4)
    n_in = [struct.unpack_from("<H", blob, off + 2)[0] for off in offs]
    bounds = [sum(n_in[:t]) for t in range(n + 1)]
    reset(engine, 512)
    rc = engine.lib.kv_utxo_upsert(ctx(engine), b"".join(op for op, _ in seeds),
                                   b"".join(e for _, e in seeds),
                                   ctypes.c_size_t(len(seeds)))
    assert rc == 0, err(engine)
    codes, _, _, token = engine.validate_block_utxo_undo(stripped, n, 10**9, block_daa,
                                                         SKIP_MASS)
    accepted = [t for t in range(n) if codes[t] == 0]
    assert 0 < len(accepted) < n
    # the host never saw this diff: the spent entries of the accepted txs, then
    # their outputs at the block's daa score
    want, scripts = [], []
    spent = [seeds[i] for t in accepted for i in range(bounds[t], bounds[t + 1])]
    removed_amount = 0
    for op, e64 in spent:
        amount, daa, flags, version, ln = struct.unpack_from("<QQHHI", e64)
        want.append(op + struct.pack("<IQQHHI", NO_QUERY, amount, daa,
                                     flags | F_REMOVED, version, ln) + bytes(32))
        scripts.append(e64[24:24 + ln])
        removed_amount += amount
    txs = block_outputs(blob, n)
    added_amount = n_created = 0
    for t in accepted:
        tx_id, outs = txs[t]
        for i, (value, version, spk, cov) in enumerate(outs):
            want.append(tx_id + struct.pack("<IIQQHHI", i, NO_QUERY, value, block_daa,
                                            F_COVENANT if cov else 0, version,
                                            len(spk)) + (cov or bytes(32)))
            scripts.append(spk)
            added_amount += value
            n_created += 1
    assert spent and n_created
    walk = Walk(engine, token, [], 256, ALL, spk_cap=1 << 16)
    assert walk.calls == 1
    assert walk.records == want and walk.scripts == scripts
    assert walk.totals == dict(
        cursor_end=len(spent) + 2 * n_created, added_amount=added_amount,
        removed_amount=removed_amount, n_added=n_created, n_removed=len(spent),
        n_added_gone=0)
    # one subscribed script: what its owner is told
    q = (struct.unpack_from("<H", spent[0][1], 18)[0], scripts[0])
    recs, spks, _, res = engine.utxo_changes_by_spk(token, [q], 8, spk_cap=MAX_SPK)
    assert recs[:36] == spent[0][0] and recs[36:40] == bytes(4)
    assert spks.startswith(scripts[0])
    assert totals(res) == walk.totals
