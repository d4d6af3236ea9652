"""Queries by script public key on the GPU-resident UTXO table:
kv_utxo_balance_by_spk ⇔ get_balance_by_script_public_keys +
get_circulating_supply, kv_utxo_find_by_spk ⇔ get_utxos_by_script_public_keys
(indexes/utxoindex/src/core/api/mod.rs:23-30).

The model is a Python dict outpoint -> Entry, independent of the engine: a
balance is a sum over the entries whose (version, script) equals the query's,
mod 2^64; a match record is packed here byte by byte. Helpers are local."""
import ctypes
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

F_COINBASE, F_ARENA, F_COVENANT = 1, 2, 4
MAX_SPK, QUERY_MAX, REC = 10000, 65536, 96
M64 = (1 << 64) - 1


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
        """the 64-byte record handed to kv_utxo_upsert_spk"""
        head = struct.pack("<QQHHI", self.amount, self.daa, self.flags(),
                           self.version, len(self.spk))
        if self.cov is not None:
            field = bytes(4) + self.cov
        elif len(self.spk) > 36:
            field = bytes(36)
        else:
            field = self.spk.ljust(36, b"\0")
        return head + field + bytes(4)

    def record(self, op36, query_index):
        """the 96-byte match record of kv_utxo_find_by_spk"""
        return (op36 + struct.pack("<IQQH", query_index, self.amount, self.daa,
                                   self.flags())
                + bytes(6) + (self.cov or bytes(32)))


def model_balances(model, queries):
    index = {q: i for i, q in enumerate(queries)}
    bal, cnt = [0] * len(queries), [0] * len(queries)
    for e in model.values():
        i = index.get((e.version, e.spk))
        if i is not None:
            bal[i] = (bal[i] + e.amount) & M64
            cnt[i] += 1
    total = sum(e.amount for e in model.values()) & M64
    return bal, cnt, total, len(model)


def model_records(model, queries):
    index = {q: i for i, q in enumerate(queries)}
    return {e.record(op, index[(e.version, e.spk)])
            for op, e in model.items() if (e.version, e.spk) in index}


# ---------------- table helpers ----------------

def ctx(engine):
    return ctypes.c_void_p(engine.ctx)


def err(engine):
    return engine.lib.kv_last_error().decode()


def reset(engine, capacity):
    assert engine.lib.kv_utxo_reset(ctx(engine), ctypes.c_uint64(capacity)) == 0


def upsert(engine, items):
    ops = b"".join(op for op, _ in items)
    ents = b"".join(e.pack() for _, e in items)
    blob = b"".join(e.spk for _, e in items if e.in_blob())
    rc = engine.lib.kv_utxo_upsert_spk(ctx(engine), ops, ents, blob,
                                       ctypes.c_size_t(len(blob)),
                                       ctypes.c_size_t(len(items)))
    assert rc == 0, err(engine)


def remove(engine, ops):
    rc = engine.lib.kv_utxo_remove(ctx(engine), b"".join(ops),
                                   ctypes.c_size_t(len(ops)))
    assert rc == 0, err(engine)


def rand_op(rng):
    return rng.randbytes(32) + struct.pack("<I", rng.randrange(8))


def check_balances(engine, model, queries):
    bal, cnt, total, n_live, ms = engine.utxo_balance_by_spk(queries)
    assert (bal, cnt, total, n_live) == model_balances(model, queries)
    assert n_live == engine.utxo_stats()["n_live"]
    assert ms >= 0.0
    return bal, cnt


class Walk:
    """a find walk with the queries packed once; .records in the order they
    came out, .cursors[i] the cursor after call i, .sizes[i] its n"""

    def __init__(self, engine, queries, max_entries, start=0):
        from rusty_kaspa_amd.engine import pack_spk_queries
        heads, blob, n_q = pack_spk_queries(queries)
        slots = engine.utxo_stats()["slots"]
        out = (ctypes.c_uint8 * (REC * max_entries))()
        cur, n = ctypes.c_uint64(start), ctypes.c_size_t()
        self.records, self.cursors, self.sizes = [], [], []
        while True:
            before = cur.value
            rc = engine.lib.kv_utxo_find_by_spk(
                ctx(engine), ctypes.byref(cur), heads, ctypes.c_size_t(n_q), blob,
                ctypes.c_size_t(len(blob)), ctypes.c_size_t(max_entries), out,
                ctypes.byref(n))
            assert rc == 0, err(engine)
            assert n.value <= max_entries and before <= cur.value <= slots
            # a call that returns nothing advances, unless at the end already
            assert n.value > 0 or cur.value > before or before == slots
            self.cursors.append(cur.value)
            self.sizes.append(n.value)
            raw = ctypes.string_at(out, REC * n.value)
            self.records += [raw[REC * i:REC * (i + 1)] for i in range(n.value)]
            if n.value == 0 and cur.value == slots:
                break
            assert len(self.cursors) <= slots + 2, "the walk did not end"
        self.calls = len(self.cursors)


def check_walk(engine, model, queries, max_entries):
    walk = Walk(engine, queries, max_entries)
    want = model_records(model, queries)
    assert len(walk.records) == len(set(walk.records)) == len(want)  # exactly once
    assert set(walk.records) == want  # byte-exact
    return walk


# ---------------- the script cases of the host test ----------------

def special_entries(rng):
    """inline, arena at 37 / 200 / 10,000 bytes, covenant entries with short
    scripts, a version-only difference, abc against abc\\0, the empty script"""
    base36 = rng.randbytes(36)
    s34, s20 = rng.randbytes(34), rng.randbytes(20)
    amount = lambda: rng.randrange(1, 1 << 50)
    daa = lambda: rng.randrange(1 << 40)
    ents = [
        Entry(amount(), daa(), s34),
        Entry(amount(), daa(), s34, coinbase=True),       # two entries, one script
        Entry(amount(), daa(), s34, version=1),           # version only
        Entry(amount(), daa(), base36),
        Entry(amount(), daa(), base36 + b"\7"),           # arena, shares the inline 36
        Entry(amount(), daa(), base36[:35]),
        Entry(amount(), daa(), rng.randbytes(200)),
        Entry(amount(), daa(), rng.randbytes(MAX_SPK)),
        Entry(amount(), daa(), b"abc"),
        Entry(amount(), daa(), b"abc\0"),
        Entry(amount(), daa(), b""),
        Entry(amount(), daa(), b"", coinbase=True),
        Entry(amount(), daa(), b"", cov=rng.randbytes(32)),   # covenant, empty
        Entry(amount(), daa(), s20, cov=rng.randbytes(32)),   # covenant, 20 bytes
        Entry(amount(), daa(), s20),                      # the same script inline
        Entry(amount(), daa(), s34, cov=rng.randbytes(32), coinbase=True),
        Entry(M64, daa(), rng.randbytes(35)),
        Entry(0, daa(), rng.randbytes(1)),
    ]
    ents += [Entry(amount(), daa(), rng.randbytes(34)) for _ in range(3)]
    return [(rand_op(rng), e) for e in ents]


def queries_of(model):
    return list(dict.fromkeys((e.version, e.spk) for e in model.values()))


def absent_queries(rng, model, n):
    have = set(queries_of(model))
    out = []
    for version, spk in list(have):
        for q in ((version + 2, spk), (version, spk + b"\1"),
                  (version, spk[:-1]) if spk else (version, b"\0")):
            if q not in have and q not in out and len(q[1]) <= MAX_SPK:
                out.append(q)
    while len(out) < n:
        q = (0, rng.randbytes(34))
        if q not in have:
            out.append(q)
    rng.shuffle(out)
    return out[:n]


# ---------------- 1: never reset, and an empty table ----------------

def test_never_reset_and_empty_table(engine):
    from rusty_kaspa_amd.engine import Engine
    queries = [(0, b"abc"), (1, b"abc"), (0, bytes(200))]
    fresh = Engine()
    try:
        for qs in (queries, []):
            assert fresh.utxo_balance_by_spk(qs) == (
                [0] * len(qs), [0] * len(qs), 0, 0, 0.0)
        assert fresh.utxo_find_by_spk(0, queries, 10) == (0, b"", 0)
        assert fresh.utxo_find_by_spk(5, queries, 10) == (5, b"", 0)  # cursor kept
    finally:
        fresh.close()
    reset(engine, 32)
    for qs in (queries, []):
        bal, cnt, total, n_live, _ = engine.utxo_balance_by_spk(qs)
        assert (bal, cnt, total, n_live) == ([0] * len(qs), [0] * len(qs), 0, 0)
    assert engine.utxo_find_by_spk(0, queries, 10) == (64, b"", 0)
    assert engine.utxo_find_by_spk(64, queries, 10) == (64, b"", 0)
    assert Walk(engine, queries, 10).records == []


# ---------------- 2: every script case in a 64-slot table ----------------

def test_small_table_every_script_case(engine):
    rng = random.Random(71)
    items = special_entries(rng)
    model = dict(items)
    assert len(model) == 21
    reset(engine, 32)
    assert engine.utxo_stats()["slots"] == 64
    upsert(engine, items)
    present = queries_of(model)
    queries = present + absent_queries(rng, model, 20)
    rng.shuffle(queries)
    bal, cnt = check_balances(engine, model, queries)
    by_q = dict(zip(queries, cnt))
    s34, s20 = items[0][1].spk, items[13][1].spk
    assert by_q[(0, s34)] == 3 and by_q[(1, s34)] == 1  # the covenant id is no key
    assert by_q[(0, s20)] == 2 and by_q[(0, b"")] == 3
    assert by_q[(0, b"abc")] == by_q[(0, b"abc\0")] == 1
    assert sum(cnt) == len(model)
    for max_entries in (1, 5, 64):
        walk = check_walk(engine, model, queries, max_entries)
        assert walk.calls <= len(model) // max_entries + 1 + 2
    # one query at a time, each alone and each absent one
    for q in present[:6] + queries[:4]:
        check_balances(engine, model, [q])
        check_walk(engine, model, [q], 3)
    # the supply alone
    check_balances(engine, model, [])
    assert engine.utxo_find_by_spk(0, [], 8) == (64, b"", 0)


# ---------------- 3 and 4: whole waves match one query ----------------

def hot_table(engine, rng):
    hot = rng.randbytes(34)
    items = [(rand_op(rng), Entry((1 << 55) - rng.randrange(1 << 20),
                                  rng.randrange(1 << 40), hot))
             for _ in range(300)]
    items += [(rand_op(rng), Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                                   rng.randbytes(rng.choice([34, 35, 60]))))
              for _ in range(100)]
    rng.shuffle(items)
    reset(engine, 512)
    assert engine.utxo_stats()["slots"] == 1024
    upsert(engine, items)
    return hot, items, dict(items)


def test_hot_script_sum_passes_2_63(engine):
    rng = random.Random(72)
    hot, items, model = hot_table(engine, rng)
    other = next(e.spk for _, e in items if e.spk != hot)
    queries = [(0, other), (0, hot), (1, hot), (0, hot + b"\0")]
    bal, cnt = check_balances(engine, model, queries)
    assert cnt[1] == 300 and (1 << 63) < bal[1] < (1 << 64)
    assert bal[2] == bal[3] == 0
    walk = Walk(engine, [(0, hot)], 64)
    assert sorted(walk.records) == sorted(model_records(model, [(0, hot)]))
    assert len(walk.records) == 300
    assert walk.sizes[:4] == [64] * 4 and sum(walk.sizes) == 300
    assert 5 <= walk.calls - 1 <= 300 // 64 + 1024 // engine.utxo_commitment_window() + 2


def test_removed_and_overwritten_entries_do_not_count(engine):
    rng = random.Random(73)
    hot, items, model = hot_table(engine, rng)
    hot_ops = [op for op, e in items if e.spk == hot]
    gone = hot_ops[::2]
    remove(engine, gone)
    for op in gone:
        del model[op]
    elsewhere = rng.randbytes(34)
    rewrites = [(op, Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                           elsewhere if i % 2 else rng.randbytes(100)))
                for i, op in enumerate(hot_ops[1::2][:40])]
    rewrites += [(op, Entry(7, 8, hot)) for op, e in items[:30] if e.spk != hot]
    upsert(engine, rewrites)
    model.update(rewrites)
    assert engine.utxo_stats()["n_tomb"] == 150
    queries = [(0, hot), (0, elsewhere)] + absent_queries(rng, model, 5)
    bal, cnt = check_balances(engine, model, queries)
    n_hot = sum(1 for e in model.values() if e.spk == hot)
    assert cnt[:2] == [n_hot, 20] and 110 < n_hot < 150
    check_walk(engine, model, queries, 64)
    check_balances(engine, model, queries_of(model))


# ---------------- 5 and 6: four scan windows ----------------

def load_four_windows(engine, seed=74):
    """Capacity 2 x window -> 4 windows of slots. About 5,000 entries: 50
    scripts hold about 90 entries each (inline, arena and covenant ones among
    them) and 500 more scripts one entry each, so that 500 of 1,000 queries
    can be present. Returns (model, queries, rng)."""
    rng = random.Random(seed)
    window = engine.utxo_commitment_window()
    reset(engine, 2 * window)
    assert engine.utxo_stats()["slots"] == 4 * window
    lens = [34] * 30 + [35] * 8 + [0, 1, 20, 36, 37, 37, 64, 200, 400, 2000, 10000, 33]
    heavy = [(i % 2, rng.randbytes(ln)) for i, ln in enumerate(lens)]
    assert len(set(heavy)) == 50
    items = []
    for k in range(4500):
        version, spk = heavy[rng.randrange(50)]
        if len(spk) > 1000 and k % 8:  # keep the arena small: few huge copies
            version, spk = heavy[0]
        cov = rng.randbytes(32) if rng.random() < 0.05 else None
        items.append((rand_op(rng), Entry(rng.randrange(1 << 50),
                                          rng.randrange(1 << 40), spk, version,
                                          rng.random() < 0.1, cov)))
    singles = [(0, rng.randbytes(rng.choice([34, 34, 35, 50]))) for _ in range(500)]
    items += [(rand_op(rng), Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                                   spk, version)) for version, spk in singles]
    model = dict(items)
    assert len(model) == len(items) == 5000
    upsert(engine, items)
    present = heavy + singles[:450]
    queries = present + absent_queries(rng, model, 500)
    rng.shuffle(queries)
    assert len(set(queries)) == 1000
    return model, queries, rng


def few_match_subset(model, queries, lo=30, hi=50):
    """queries whose matches number about 40"""
    _, cnt, _, _ = model_balances(model, queries)
    picked, n = [], 0
    for q, c in sorted(zip(queries, cnt), key=lambda t: t[1]):
        if c and n + c <= hi:
            picked.append(q)
            n += c
    assert lo <= n <= hi
    return picked + [q for q, c in zip(queries, cnt) if c == 0][:5], n


def test_four_windows_balances_and_walks(engine):
    model, queries, rng = load_four_windows(engine)
    window = engine.utxo_commitment_window()
    slots = 4 * window
    bal, cnt = check_balances(engine, model, queries)
    n_match = sum(cnt)
    assert sum(1 for c in cnt if c) == 500 and n_match > 4500
    walks = {}
    for max_entries in (7, 4096):
        walks[max_entries] = walk = check_walk(engine, model, queries, max_entries)
        assert walk.calls <= n_match // max_entries + slots // window + 2
    subset, n_few = few_match_subset(model, queries)
    walk = check_walk(engine, model, subset, 1)
    assert walk.calls <= n_few + slots // window + 2
    assert walks[7].records == walks[4096].records  # slot order both times
    # a walk from a cursor inside the second window: what the full walk gave
    # from that cursor on
    full = walks[7]
    inside = [i for i, c in enumerate(full.cursors)
              if window < c < 2 * window and c % window]
    assert inside
    i = inside[len(inside) // 2]
    rest = full.records[sum(full.sizes[:i + 1]):]
    for max_entries in (7, 4096):
        part = Walk(engine, queries, max_entries, start=full.cursors[i])
        assert part.records == rest
    assert 0 < len(rest) < len(full.records)


def test_after_rehash_and_after_a_reverted_diff(engine):
    model, queries, rng = load_four_windows(engine, seed=75)
    gone = rng.sample(list(model), 1500)  # leave tombstones and arena garbage
    remove(engine, gone)
    for op in gone:
        del model[op]
    bal0, cnt0 = check_balances(engine, model, queries)
    rec0 = set(check_walk(engine, model, queries, 4096).records)
    st = engine.utxo_stats()
    assert st["arena_used"] > st["arena_live_bytes"] > 0
    engine.utxo_rehash(0)  # arena offsets and slots move
    st = engine.utxo_stats()
    assert st["arena_used"] == st["arena_live_bytes"] and st["n_tomb"] == 0
    assert check_balances(engine, model, queries) == (bal0, cnt0)
    assert set(check_walk(engine, model, queries, 4096).records) == rec0
    # a journaled diff: remove 200, add 200 on scripts old and new
    removed = rng.sample(list(model), 200)
    q_scripts = [q for q, c in zip(queries, cnt0) if c][:40]
    added = [(rand_op(rng), Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                                  spk, version,
                                  cov=rng.randbytes(32) if k % 7 == 0 else None))
             for k, (version, spk) in enumerate(q_scripts * 5)]
    token, _ = engine.utxo_apply_diff(
        b"".join(removed), b"".join(op for op, _ in added),
        b"".join(e.pack() for _, e in added),
        b"".join(e.spk for _, e in added if e.in_blob()))
    after = {op: e for op, e in model.items() if op not in set(removed)}
    after.update(added)
    bal1, cnt1 = check_balances(engine, after, queries)
    assert (bal1, cnt1) != (bal0, cnt0)
    check_walk(engine, after, queries, 4096)
    engine.utxo_revert(token)
    assert check_balances(engine, model, queries) == (bal0, cnt0)
    assert set(check_walk(engine, model, queries, 4096).records) == rec0


# ---------------- 7: refusals ----------------

PATTERN = 0xA5


def raw_balance(engine, heads, n_q, blob, blob_len):
    from rusty_kaspa_amd.engine import KvSpkQuery
    arr = (KvSpkQuery * max(len(heads), 1))(*[KvSpkQuery(*h) for h in heads])
    m = max(min(n_q, 8), 1)
    bal = (ctypes.c_uint64 * m)(*[PATTERN] * m)
    cnt = (ctypes.c_uint64 * m)(*[PATTERN] * m)
    total, n_live = ctypes.c_uint64(PATTERN), ctypes.c_uint64(PATTERN)
    ms = ctypes.c_double(-1.0)
    rc = engine.lib.kv_utxo_balance_by_spk(
        ctx(engine), arr, ctypes.c_size_t(n_q), blob, ctypes.c_size_t(blob_len),
        bal, cnt, ctypes.byref(total), ctypes.byref(n_live), ctypes.byref(ms))
    untouched = (list(bal) == [PATTERN] * m and list(cnt) == [PATTERN] * m
                 and total.value == n_live.value == PATTERN and ms.value == -1.0)
    return rc, untouched


def raw_find(engine, heads, n_q, blob, blob_len):
    from rusty_kaspa_amd.engine import KvSpkQuery
    arr = (KvSpkQuery * max(len(heads), 1))(*[KvSpkQuery(*h) for h in heads])
    out = (ctypes.c_uint8 * (REC * 4))(*[PATTERN] * (REC * 4))
    cur, n = ctypes.c_uint64(3), ctypes.c_size_t(PATTERN)
    rc = engine.lib.kv_utxo_find_by_spk(
        ctx(engine), ctypes.byref(cur), arr, ctypes.c_size_t(n_q), blob,
        ctypes.c_size_t(blob_len), ctypes.c_size_t(4), out, ctypes.byref(n))
    untouched = (bytes(out) == bytes([PATTERN]) * (REC * 4) and cur.value == 3
                 and n.value == PATTERN)
    return rc, untouched


def test_refusals_write_nothing(engine):
    rng = random.Random(76)
    items = special_entries(rng)
    reset(engine, 32)
    upsert(engine, items)
    s34 = items[0][1].spk
    c0 = engine.utxo_commitment()[:2]
    cases = {
        "duplicate": ([(34, 0, 0), (3, 0, 0), (34, 0, 0)], 3, s34 + b"abc" + s34, 71),
        "over-long script": ([(34, 0, 0), (MAX_SPK + 1, 0, 0)], 2,
                             s34 + bytes(MAX_SPK + 1), 34 + MAX_SPK + 1),
        "too many queries": ([(0, 0, 0)], QUERY_MAX + 1, b"", 0),
        "blob too long": ([(34, 0, 0)], 1, s34 + b"\0", 35),
        "blob too short": ([(34, 0, 0), (3, 0, 0)], 2, s34 + b"abc", 36),
        "non-zero zero field": ([(34, 0, 0), (3, 0, 1)], 2, s34 + b"abc", 37),
    }
    for name, (heads, n_q, blob, blob_len) in cases.items():
        assert raw_balance(engine, heads, n_q, blob, blob_len) == (-1, True), name
        assert err(engine), name
        assert raw_find(engine, heads, n_q, blob, blob_len) == (-1, True), name
        assert err(engine), name
    with pytest.raises(RuntimeError):
        engine.utxo_balance_by_spk([(0, s34), (0, s34)])
    with pytest.raises(RuntimeError):
        engine.utxo_find_by_spk(0, [(0, s34), (0, s34)], 4)
    # the same arguments, mended, are served; the set is as it was
    rc, untouched = raw_balance(engine, [(34, 0, 0), (3, 0, 0)], 2, s34 + b"abc", 37)
    assert (rc, untouched) == (0, False)
    rc, untouched = raw_find(engine, [(34, 0, 0), (3, 0, 0)], 2, s34 + b"abc", 37)
    assert (rc, untouched) == (0, False)
    assert engine.utxo_commitment()[:2] == c0


def test_the_largest_query_set(engine):
    """n_q = KV_UTXO_QUERY_MAX distinct 34-byte scripts, a few of them present"""
    rng = random.Random(77)
    items = [(rand_op(rng), Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                                  rng.randbytes(34))) for _ in range(40)]
    model = dict(items)
    reset(engine, 64)
    upsert(engine, items)
    queries = [(0, struct.pack("<I", i) + bytes(30)) for i in range(QUERY_MAX - 40)]
    queries += queries_of(model)
    assert len(set(queries)) == QUERY_MAX
    bal, cnt = check_balances(engine, model, queries)
    assert sum(cnt) == 40 and cnt[:QUERY_MAX - 40] == [0] * (QUERY_MAX - 40)
    cursor, recs, n = engine.utxo_find_by_spk(0, queries, 64)
    assert n == 40 and cursor == 128
    assert {recs[REC * i:REC * (i + 1)] for i in range(n)} == \
        model_records(model, queries)
